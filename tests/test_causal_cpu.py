"""CPU tests (no GPU) of the causal (time-weighted) residual loss: (a) the fp64 model `causal_model.py` against torch
autograd of its own definition; (b) the fp32 bin formula in its numpy and torch spellings; (c) the properties the
definition promises; (d) the host checks of `pinn_causal_weights` through the C ABI (the library loads without a GPU and
these return before any HIP call) and its declaration / export; (e) the config; (f) the trainer's routing."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import pinnrl_amd  # noqa: F401
import causal_model as CM
from pinnrl_amd import _lib
from pinnrl_amd import engine as E
from pinnrl_amd import pdes as P
from pinnrl_amd.config import AdaptiveWeightsConfig, CausalWeightingConfig, Config, TrainingConfig
from pinnrl_amd.pdes.pde_base import causal_bins, causal_residual_loss
from pinnrl_amd.training import PDETrainer

T_LO, T_HI = 0.25, 2.0


def _inputs(N, seed, delta=0.5):
    """Residuals with exact zeros and |r| = delta among them (the kinks of mae and huber), times over and around the domain."""
    g = np.random.default_rng(seed)
    r = g.standard_normal(N).astype(np.float32)
    r[::7] = 0.0
    r[3::11] = np.float32(delta)
    r[5::13] = -np.float32(delta)
    t = g.uniform(T_LO - 0.05, T_HI + 0.05, N).astype(np.float32)
    return r, t


def _edge_times(M, lo=T_LO, hi=T_HI):
    """t_lo, t_hi, every interior bin edge as torch.linspace gives it in fp32, and points outside the domain."""
    edges = torch.linspace(lo, hi, M + 1, dtype=torch.float32).numpy()
    out = np.array([lo - 1.0, lo - 1e-6, hi + 1e-6, hi + 3.0, np.nextafter(np.float32(lo), np.float32(-9)),
                    np.nextafter(np.float32(hi), np.float32(9))], dtype=np.float32)
    near = np.concatenate([np.nextafter(edges, np.float32(-9)), np.nextafter(edges, np.float32(9))]).astype(np.float32)
    return np.concatenate([edges, out, near]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model's cotangent is the gradient of its loss
# ---------------------------------------------------------------------------------------------------------------------
def _torch_pointwise(r, loss, delta):
    if loss == "mae":
        return r.abs()
    if loss == "huber":
        d = float(np.float32(delta))
        a = r.abs()
        return torch.where(a < d, 0.5 * r * r, d * (a - 0.5 * d))
    return r * r


@pytest.mark.parametrize("M", [1, 7, 16])
@pytest.mark.parametrize("loss", CM.LOSSES)
def test_model_cotangent_is_autograd_of_the_loss_with_detached_weights(loss, M):
    delta, gs, eps = 0.5, 0.37, 0.8
    r32, t32 = _inputs(301, 1, delta)
    m = CM.causal_model(r32, t32, eps, M, T_LO, T_HI, loss, delta, grad_scale=gs)
    r = torch.from_numpy(r32).double().requires_grad_(True)
    w = torch.from_numpy(m.w)[torch.from_numpy(m.bins).long()]  # detached: constants of the differentiation
    total = float(np.float32(gs)) * (w * _torch_pointwise(r, loss, delta)).sum()
    g, = torch.autograd.grad(total, r)
    # torch's abs has sgn(0) = 0 and `where` takes the quadratic branch on |r| < delta: the kernel's conventions
    np.testing.assert_allclose(m.rbar, g.numpy(), rtol=1e-15, atol=0.0)
    assert np.all(m.rbar[r32 == 0.0] == 0.0)
    assert m.L_total == pytest.approx(float((w * _torch_pointwise(r, loss, delta)).sum().detach()) / r32.size, rel=1e-14)
    # the definition, spelt out bin by bin
    for i in range(M):
        sel = m.bins == i
        assert m.c[i] == sel.sum()
        assert m.S[i] == pytest.approx(float(CM.loss_value(r32[sel], loss, delta).sum()), rel=1e-13, abs=0.0)
        assert m.L[i] == (m.S[i] / m.c[i] if m.c[i] else 0.0)
        assert m.w_exact[i] == pytest.approx(math.exp(-float(np.float32(eps)) * float(m.L[:i].sum())), rel=1e-14)


@pytest.mark.parametrize("loss", CM.LOSSES)
def test_eager_formula_of_pde_base_is_the_model(loss):
    """`causal_residual_loss` (the autograd path of PDEBase._residual_loss) computes the model's L and weights."""
    delta, M, eps = 0.5, 8, 1.3
    r32, t32 = _inputs(257, 2, delta)
    m = CM.causal_model(r32, t32, eps, M, T_LO, T_HI, loss, delta)
    r = torch.from_numpy(r32).double().requires_grad_(True)
    L, w = causal_residual_loss(_torch_pointwise(r, loss, delta), torch.from_numpy(t32), M, float(np.float32(eps)), T_LO, T_HI)
    assert w.dtype == torch.float32 and not w.requires_grad
    np.testing.assert_array_equal(w.numpy().astype(np.float64), m.w)
    assert float(L.detach()) == pytest.approx(m.L_total, rel=1e-13)
    g, = torch.autograd.grad(L * r32.size, r)
    np.testing.assert_allclose(g.numpy(), m.rbar, rtol=1e-14, atol=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# (b) bins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(T_LO, T_HI), (0.0, 1.0), (-0.3, 0.7), (0.0, 100.0)])
@pytest.mark.parametrize("M", [1, 2, 3, 7, 8, 16, 50, 64])
def test_bins_agree_between_the_spellings_and_stay_in_range(M, lo, hi):
    t = _edge_times(M, lo, hi)
    b_np = CM.bins(t, M, lo, hi)
    b_t = causal_bins(torch.from_numpy(t), M, lo, hi)
    assert b_t.dtype == torch.int32 and b_np.dtype == np.int32
    np.testing.assert_array_equal(b_np, b_t.numpy())
    assert b_np.min() >= 0 and b_np.max() <= M - 1
    edges = t[: M + 1]
    assert b_np[0] == 0 and b_np[M] == M - 1  # t_lo: first bin; t_hi: last bin
    assert np.all(np.diff(b_np[: M + 1]) >= 0)  # monotone over the edges
    below = t < np.float32(lo)
    assert np.all(b_np[below] == 0) and np.all(b_np[t >= np.float32(hi)] == M - 1)
    # the spelt-out formula: one rounded fp32 operation each
    s = np.float32(np.float64(M) / (np.float64(hi) - np.float64(lo)))
    for tv, bv in zip(t.tolist(), b_np.tolist()):
        v = np.float32(np.float32(np.float32(tv) - np.float32(lo)) * s)
        assert bv == int(min(max(v, np.float32(0)), np.float32(M - 1)))
    assert edges.size == M + 1


def test_bins_of_the_uniform_grid_of_the_sampler():
    """A floor(sqrt(N))-point linspace of the time domain puts many points exactly on bin edges: both spellings agree there."""
    for G in (10, 16, 64, 223):
        t = torch.linspace(0.0, 1.0, G, dtype=torch.float32)
        for M in (8, 16, 64):
            np.testing.assert_array_equal(CM.bins(t.numpy(), M, 0.0, 1.0), causal_bins(t, M, 0.0, 1.0).numpy())


# ---------------------------------------------------------------------------------------------------------------------
# (c) properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", CM.LOSSES)
def test_zero_sharpness_and_one_bin_give_the_plain_loss(loss):
    r, t = _inputs(500, 3)
    plain = float(CM.loss_value(r, loss, 0.5).sum()) / r.size
    for M, eps in ((9, 0.0), (1, 5.0), (1, 0.0)):
        m = CM.causal_model(r, t, eps, M, T_LO, T_HI, loss, 0.5, grad_scale=0.25)
        assert np.all(m.w == 1.0)
        assert m.L_total == pytest.approx(plain, rel=1e-14) and m.plain_total == pytest.approx(plain, rel=1e-14)
        np.testing.assert_array_equal(m.rbar, 0.25 * CM.loss_derivative(r, loss, 0.5))


def test_a_sharpness_that_underflows_gives_exact_zeros():
    M = 8
    t = np.linspace(T_LO, T_HI, 400, endpoint=False).astype(np.float32)
    r = np.ones(400, dtype=np.float32)
    b = CM.bins(t, M, T_LO, T_HI)
    r[b < 2] = 0.0  # the first two bins carry no loss: the first non-zero L_k is L_2
    m = CM.causal_model(r, t, 1e30, M, T_LO, T_HI)
    assert np.all(m.w[:3] == 1.0) and np.all(m.w[3:] == 0.0)
    assert np.all(m.rbar[b >= 3] == 0.0) and np.all(m.rbar[b == 2] == 2.0)
    assert m.L_total == pytest.approx(float((b == 2).sum()) / 400.0)


def test_empty_bins_contribute_nothing_and_do_not_shift_later_weights():
    M, eps = 8, 0.7
    g = np.random.default_rng(4)
    width = (T_HI - T_LO) / M
    keep = [0, 1, 4, 7]  # bins 2, 3, 5, 6 stay empty
    t = np.concatenate([g.uniform(T_LO + (k + 0.1) * width, T_LO + (k + 0.9) * width, 40) for k in keep]).astype(np.float32)
    r = g.standard_normal(t.size).astype(np.float32)
    m = CM.causal_model(r, t, eps, M, T_LO, T_HI)
    assert [int(c) for c in m.c] == [40, 40, 0, 0, 40, 0, 0, 40]
    assert np.all(m.L[[2, 3, 5, 6]] == 0.0) and np.all(m.S[[2, 3, 5, 6]] == 0.0)
    assert m.w[2] == m.w[3] == m.w[4] and m.w[5] == m.w[6] == m.w[7]
    # the same points in a 4-bin layout without the gaps: the occupied bins keep their weights
    dense = CM.causal_model(r, (np.repeat(np.arange(4), 40) + 0.5).astype(np.float32), eps, 4, 0.0, 4.0)
    np.testing.assert_array_equal(m.w[keep], dense.w)
    assert m.L_total == pytest.approx(dense.L_total, rel=1e-15)  # numpy sums the eight and the four terms in its own order


# ---------------------------------------------------------------------------------------------------------------------
# (d) the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _call(N=8, n_bins=4, t_lo=0.0, t_hi=1.0, loss=0, residual=0x1000, t=0x1000, eps=0x1000, cot=0x1000, weights=0x1000,
          scratch=0x1000):
    """pinn_causal_weights with made-up device addresses: every case below must be answered before any HIP call."""
    return _lib.load().pinn_causal_weights(residual, t, N, n_bins, t_lo, t_hi, eps, loss, 1.0, 1.0, cot, None, None, None, weights,
                                           scratch, None)


def test_symbol_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pinn_jet.h")).read()
    assert re.search(r"\bint pinn_causal_weights\s*\(", hdr)
    assert "pinn_causal_weights" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "pinn_causal_weights")
    assert lib.pinn_abi_version() == 2 == _lib.PINN_ABI_VERSION  # additive: the version stays
    assert re.search(r"#define PINN_CAUSAL_MAX_BINS 64\b", hdr) and _lib.PINN_CAUSAL_MAX_BINS == 64
    assert re.search(r"#define PINN_CAUSAL_SCRATCH_DOUBLES \(64 \* 2 \* PINN_CAUSAL_MAX_BINS\)", hdr)
    assert _lib.PINN_CAUSAL_SCRATCH_DOUBLES == 64 * 2 * 64
    assert CausalWeightingConfig.MAX_BINS == _lib.PINN_CAUSAL_MAX_BINS


def test_validation_cases_are_answered_on_the_host():
    lib = _lib.load()
    BAD, MIS = -1, -3

    def err():
        return lib.pinn_last_error().decode()

    assert _call(N=0) == 0  # no-op, whatever the pointers
    assert _call(N=0, residual=None, t=None, eps=None, cot=None, weights=None, scratch=None) == 0
    for m in (0, -1, 65, 1 << 20):
        assert _call(n_bins=m) == BAD and "n_bins" in err(), m
    for lo, hi in ((0.0, 0.0), (1.0, 0.5), (0.0, math.inf), (-math.inf, 1.0), (math.nan, 1.0), (0.0, math.nan)):
        assert _call(t_lo=lo, t_hi=hi) == BAD and "time domain" in err(), (lo, hi)
        assert _call(N=0, t_lo=lo, t_hi=hi) == BAD  # the descriptor is checked before the empty batch is accepted
    for kind in (-1, 3, 99):
        assert _call(loss=kind) == BAD and "loss" in err(), kind
    assert _call(N=-1) == BAD and "N < 0" in err()
    for name in ("residual", "t", "eps", "cot", "weights", "scratch"):
        assert _call(**{name: None}) == BAD and "null" in err(), name
    assert _call(scratch=0x1004) == MIS and "8-byte" in err()
    for m in (1, 64):  # the limits themselves pass the checks
        assert _call(N=0, n_bins=m) == 0


def test_engine_front_end_checks_its_arguments():
    with pytest.raises(RuntimeError, match="ROCm device"):  # no CPU fallback
        E.causal_weights(torch.zeros(8), torch.zeros(8), 4, 0.0, 1.0, torch.zeros(1), "mse", 1.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# (e) config
# ---------------------------------------------------------------------------------------------------------------------
def test_config_defaults_are_disabled():
    tc = TrainingConfig()
    cw = tc.causal_weighting
    assert isinstance(cw, CausalWeightingConfig) and cw.enabled is False and cw.num_bins == 16 and cw.eps == 1.0
    assert tc.get("causal_weighting") is cw and tc["causal_weighting"] is cw


def test_config_takes_the_dict_form_and_validates():
    tc = TrainingConfig(causal_weighting={"enabled": True, "num_bins": 8, "eps": 2.5})
    assert isinstance(tc.causal_weighting, CausalWeightingConfig)
    assert (tc.causal_weighting.enabled, tc.causal_weighting.num_bins, tc.causal_weighting.eps) == (True, 8, 2.5)
    assert CausalWeightingConfig(num_bins=1).num_bins == 1 and CausalWeightingConfig(num_bins=64, eps=0).eps == 0.0
    for bad in (0, 65, -3, 2.5, "8", True):
        with pytest.raises(ValueError, match="num_bins"):
            CausalWeightingConfig(enabled=True, num_bins=bad)
    for bad in (-1e-9, math.inf, math.nan, "x", None):
        with pytest.raises(ValueError, match="eps"):
            CausalWeightingConfig(enabled=True, eps=bad)
    with pytest.raises(ValueError, match="num_bins"):
        TrainingConfig(causal_weighting={"enabled": True, "num_bins": 100})


def _pde_config(training=None, trainable=(), observation=None):
    return P.PDEConfig(
        name="burgers", domain=[(-1.0, 1.0)], time_domain=(0.0, 1.0), parameters={"nu": 0.02},
        boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0}, exact_solution={}, dimension=1,
        device=torch.device("cpu"), training=training, trainable_parameters=list(trainable),
        parameter_initial_guesses={k: 0.05 for k in trainable}, observation_data=observation)


def test_the_pde_learns_of_it_through_the_training_config():
    on = TrainingConfig(causal_weighting=CausalWeightingConfig(enabled=True, num_bins=8, eps=0.5))
    assert P.BurgersEquation(_pde_config(on))._causal_weighting() == (8, 0.5)
    assert P.BurgersEquation(_pde_config(TrainingConfig()))._causal_weighting() is None
    assert P.BurgersEquation(_pde_config(None))._causal_weighting() is None
    as_dict = {"loss_function": "mse", "causal_weighting": {"enabled": True, "num_bins": 4, "eps": 2.0}}
    assert P.BurgersEquation(_pde_config(as_dict))._causal_weighting() == (4, 2.0)
    assert P.BurgersEquation(_pde_config({"causal_weighting": {"enabled": False}}))._causal_weighting() is None
    with pytest.raises(ValueError, match="num_bins"):
        P.BurgersEquation(_pde_config({"causal_weighting": {"enabled": True, "num_bins": 65}}))._causal_weighting()


# ---------------------------------------------------------------------------------------------------------------------
# (f) routing
# ---------------------------------------------------------------------------------------------------------------------
BURGERS_TERMS = [(1.0, ("u_t",)), (1.0, ("u", "u_x")), ((-1.0, "nu"), ("u_xx",))]


def _cfg(causal=True, kind="adam", adaptive=None, mode="forward"):
    cfg = Config.__new__(Config)
    cfg.device = torch.device("cpu")
    cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, optimizer=kind, mode=mode)
    if causal:
        cfg.training.causal_weighting = CausalWeightingConfig(enabled=True, num_bins=8, eps=1.0)
    if adaptive:
        cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy=adaptive, alpha=0.7, eps=1e-6)
    return cfg


def _trainer(cfg, term=False, process_group=None, **kw):
    pc = _pde_config(training=cfg.training, **kw)
    pde = P.TermPDE(pc, BURGERS_TERMS) if term else P.BurgersEquation(pc)
    tr = PDETrainer(torch.nn.Linear(2, 1), pde, {}, cfg, device=torch.device("cpu"), process_group=process_group)
    return tr


@pytest.mark.parametrize("term", [False, True])
def test_forward_adam_causal_takes_the_launch_list(term):
    tr = _trainer(_cfg(), term=term)
    assert tr._causal == (8, 1.0)
    assert tr._manual_step_unsupported() is None


OBS = {"x": [0.0, 0.5], "t": [0.1, 0.2], "u": [0.0, 0.1]}
COMBOS = [
    (dict(adaptive="rbw"), {}, "causal weighting with adaptive loss weights"),
    (dict(adaptive="lrw"), {}, "causal weighting with adaptive loss weights"),
    (dict(), dict(trainable=["nu"]), "causal weighting with trainable PDE coefficients"),
    (dict(mode="data_augmented"), dict(observation=OBS), "causal weighting with a data mode"),
    (dict(mode="inverse"), dict(observation=OBS), "causal weighting with"),
    (dict(mode="data_only"), dict(observation=OBS), "causal weighting with a data mode"),
]


@pytest.mark.parametrize("term", [False, True])
@pytest.mark.parametrize("cfg_kw,pde_kw,reason", COMBOS)
def test_combinations_outside_the_chain_name_their_reason(cfg_kw, pde_kw, reason, term):
    why = _trainer(_cfg(**cfg_kw), term=term, **pde_kw)._manual_step_unsupported()
    assert why is not None and why.startswith(reason), why


@pytest.mark.parametrize("term", [False, True])
@pytest.mark.parametrize("cfg_kw,pde_kw,reason", COMBOS)
def test_with_the_option_off_the_routing_is_what_it_was(cfg_kw, pde_kw, reason, term):
    """Off: the answer does not mention the option, and equals the answer of a config that never heard of it."""
    off = _trainer(_cfg(causal=False, **cfg_kw), term=term, **pde_kw)
    assert off._causal is None
    why = off._manual_step_unsupported()
    assert why is None or "causal" not in why
    bare = _cfg(causal=False, **cfg_kw)
    del bare.training.causal_weighting  # a training config of before the option (the reference's own objects)
    assert _trainer(bare, term=term, **pde_kw)._manual_step_unsupported() == why
    # and what the parent pinned for these configurations
    if cfg_kw.get("adaptive"):
        assert why is None
    elif pde_kw.get("trainable"):
        assert (why is None) != term  # a compiled PDE has the inverse launch list, a term residual names its own reason
    elif cfg_kw.get("mode") == "data_only":
        assert why is not None and "data" in why


def test_plain_forward_adam_off_is_still_covered():
    for term in (False, True):
        assert _trainer(_cfg(causal=False), term=term)._manual_step_unsupported() is None


@pytest.mark.parametrize("kind", ["lbfgs", "adam_lbfgs"])
def test_construction_refuses_lbfgs(kind):
    with pytest.raises(NotImplementedError, match="causal weighting with L-BFGS"):
        _trainer(_cfg(kind=kind))
    _trainer(_cfg(causal=False, kind=kind))  # off: built as before


def test_construction_refuses_a_process_group():
    with pytest.raises(NotImplementedError, match="causal weighting under a process group"):
        _trainer(_cfg(), process_group=object())


def test_setter_validates_and_reaches_the_config():
    tr = _trainer(_cfg())
    tr.set_causal_eps(3.5)
    assert tr._causal == (8, 3.5) and tr.config.training.causal_weighting.eps == 3.5
    assert tr.pde._causal_weighting() == (8, 3.5)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="eps"):
            tr.set_causal_eps(bad)
    assert tr.causal_weights().tolist() == [1.0] * 8  # before the first step
    off = _trainer(_cfg(causal=False))
    with pytest.raises(RuntimeError, match="not enabled"):
        off.set_causal_eps(1.0)
    with pytest.raises(RuntimeError, match="not enabled"):
        off.causal_weights()


# ---------------------------------------------------------------------------------------------------------------------
# (g) the loss every `compute_loss` trains on, with a stubbed residual (no engine: CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _stub_residual(pde, r32):
    """`compute_residual` returns r32 * scale with `scale` a leaf, so that the loss is differentiable in it."""
    scale = torch.ones((), dtype=torch.float32, requires_grad=True)
    pde.compute_residual = lambda model, x, t: torch.from_numpy(r32).reshape(-1, 1) * scale
    return scale


def _causal_training(loss="mse", delta=1.0, M=4, eps=50.0, **kw):
    return TrainingConfig(loss_function=loss, huber_delta=delta, causal_weighting=CausalWeightingConfig(enabled=True, num_bins=M, eps=eps),
                          **kw)


@pytest.mark.parametrize("kind,trainable", [("compiled", ()), ("compiled", ("nu",)), ("term", ()), ("term", ("nu",))])
def test_residual_loss_is_the_weighted_one_whatever_the_pde_and_its_coefficients(kind, trainable):
    """r = 1 everywhere, 4 bins, eps = 50: the weights are (1, e^-50, ...), so the loss is the first bin's share, 0.25 —
    also for a TermPDE with a trainable term coefficient, whose own `_residual_loss` must not return the plain mean 1."""
    tc = _causal_training()
    pc = _pde_config(training=tc, trainable=trainable)
    pde = P.TermPDE(pc, BURGERS_TERMS) if kind == "term" else P.BurgersEquation(pc)
    assert pde._has_trainable_coefficients() == bool(trainable)
    t = (torch.arange(400, dtype=torch.float32).reshape(-1, 1) + 0.5) / 400.0
    _stub_residual(pde, np.ones(400, dtype=np.float32))
    L = pde._residual_loss(torch.nn.Linear(2, 1), torch.zeros(400, 1), t)
    assert float(L.detach()) == pytest.approx(0.25, rel=1e-6)
    w = pde._causal_last_weights
    assert w[0] == 1.0 and float(w[1]) == pytest.approx(math.exp(-50.0), rel=1e-6)
    # through compute_loss and the trainer's view of the weights
    cfg = _cfg()
    cfg.training = tc
    tr = PDETrainer(torch.nn.Linear(2, 1), pde, {}, cfg, device=torch.device("cpu"))
    if trainable:
        assert tr._manual_step_unsupported().startswith("causal weighting with trainable PDE coefficients")
    out = pde.compute_loss(torch.nn.Linear(2, 1), torch.zeros(400, 1), t)
    assert float(out["residual"].detach()) == pytest.approx(0.25, rel=1e-6)
    assert tr.causal_weights()[1] < 1e-20
    tc.causal_weighting.enabled = False  # off: the plain mean again
    if not trainable:  # (the fused launch of the plain path needs the engine)
        return
    assert float(pde._residual_loss(torch.nn.Linear(2, 1), torch.zeros(400, 1), t).detach()) == pytest.approx(1.0, rel=1e-6)


@pytest.mark.parametrize("loss,delta", [("mse", 1.0), ("mae", 1.0), ("huber", 0.5)])
def test_residual_loss_of_the_eager_path_is_the_model(loss, delta):
    """`_pointwise_loss` inside `_residual_loss`: value, weights and the gradient through the residual against the model."""
    M, eps = 8, 1.3
    r32, t32 = _inputs(257, 6, delta)
    t32 = np.clip((t32 - T_LO) / (T_HI - T_LO), -0.02, 1.02).astype(np.float32)  # the PDE's time domain is (0, 1)
    pde = P.BurgersEquation(_pde_config(training=_causal_training(loss, delta, M, eps)))
    scale = _stub_residual(pde, r32)
    L = pde._residual_loss(torch.nn.Linear(2, 1), torch.zeros(257, 1), torch.from_numpy(t32).reshape(-1, 1))
    m = CM.causal_model(r32, t32, eps, M, 0.0, 1.0, loss, delta)
    # fp32 point losses and an fp32 sum of 257 terms against the model's double: (257 + 3) roundings at most
    assert float(L.detach()) == pytest.approx(m.L_total, rel=260 * 2.0 ** -24)
    # the eager path takes l(r) in fp32 (at most two roundings: relative 2^-23), so a prefix P_i is off by 2^-23 P_i and the
    # weight by eps P_i 2^-23, plus its own rounding to fp32
    w = pde._causal_last_weights.numpy().astype(np.float64)
    bound = (float(np.float32(eps)) * m.P + 1.0) * 2.0 ** -23
    assert np.all(np.abs(w - m.w_exact) <= bound * m.w_exact), (np.abs(w - m.w_exact) / m.w_exact, bound)
    g, = torch.autograd.grad(L, scale)  # dL/dscale = (1/N) sum_n w l'(r_n) r_n
    want = float(np.sum(m.rbar * r32.astype(np.float64))) / 257.0
    scale_of_sum = float(np.sum(np.abs(m.rbar * r32.astype(np.float64)))) / 257.0
    assert abs(float(g) - want) <= 260 * 2.0 ** -24 * scale_of_sum


def test_a_smoothness_term_keeps_the_causal_step_on_autograd():
    weights = {"residual": 15.0, "boundary": 20.0, "initial": 10.0, "smoothness": 0.1}

    def heat(w, causal):
        cfg = Config.__new__(Config)
        cfg.device = torch.device("cpu")
        cfg.training = TrainingConfig(learning_rate=1e-3, loss_weights=dict(w),
                                      causal_weighting=CausalWeightingConfig(enabled=causal, num_bins=8, eps=1.0))
        pde = P.HeatEquation(P.PDEConfig(
            name="heat", domain=[(0.0, 2.0)], time_domain=(0.0, 1.0), parameters={"alpha": 0.01},
            boundary_conditions={"periodic": {}}, initial_condition={"type": "sine", "amplitude": 1.0, "frequency": 2.0},
            exact_solution={}, dimension=1, device=torch.device("cpu"), training=cfg.training))
        return PDETrainer(torch.nn.Linear(2, 1), pde, {}, cfg, device=torch.device("cpu"))

    assert heat(weights, True)._manual_step_unsupported() == "causal weighting with a smoothness term"
    assert heat(weights, False)._manual_step_unsupported() is None  # off: the smoothness chain of the launch list, as before
    assert heat(dict(weights, smoothness=0.0), True)._manual_step_unsupported() is None  # no smoothness weight: the causal chain


def test_the_trainer_reads_the_settings_where_the_pde_reads_them():
    tr = _trainer(_cfg())
    tr.config.training.causal_weighting.eps = 2.0  # edited after construction: one source, so both paths see it
    assert tr._causal == (8, 2.0) == tr.pde._causal_weighting()
    tr.config.training.causal_weighting.enabled = False
    assert tr._causal is None and tr._manual_step_unsupported() is None
    # the launch list's device scalar follows an edit at its next eager step; the bin count is fixed by its buffers
    F = {"causal_host": (8, 1.0), "causal_eps": torch.tensor([1.0])}
    tr._sync_causal_state(F, (8, 2.0))
    assert F["causal_eps"].tolist() == [2.0] and F["causal_host"] == (8, 2.0)
    with pytest.raises(RuntimeError, match="num_bins changed"):
        tr._sync_causal_state(F, (16, 2.0))
    with pytest.raises(RuntimeError, match="was enabled"):
        tr._sync_causal_state({}, (8, 2.0))
