"""L-BFGS on the autograd-free step, the parts that need no GPU:
(a) the C ABI declares the new entry points, `_lib.EXPORTS` lists them, the library loads them typed and is still ABI 2;
(b) `LBFGSDriver` — torch's `step()` and strong-Wolfe control flow restated on scalars — over the fp64 model backend of
    tests/lbfgs_model.py takes the same number of function evaluations as torch.optim.LBFGS and ends at the same theta;
(c) `_manual_step_unsupported()` names each combination the flat L-BFGS does not cover."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import lbfgs_model as LM
import pinnrl_amd  # noqa: F401
from pinnrl_amd import _lib
from pinnrl_amd import pdes as P
from pinnrl_amd.config import AdaptiveWeightsConfig, Config, TrainingConfig
from pinnrl_amd.training import PDETrainer
from pinnrl_amd.training.lbfgs import LBFGSDriver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pinn_lbfgs_state_bytes", "pinn_lbfgs_scratch_bytes", "pinn_lbfgs_direction", "pinn_lbfgs_eval_stats")


# ---------------------------------------------------------------------------------------------------------------------
# (a) ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_library_agree():
    header = open(os.path.join(ROOT, "include", "pinn_jet.h")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in pinn_jet.h"
        assert name in _lib.EXPORTS
    assert re.search(r"#define\s+PINN_ABI_VERSION\s+2\b", header)
    assert int(re.search(r"#define\s+PINN_LBFGS_MAX_HISTORY\s+(\d+)", header).group(1)) == _lib.PINN_LBFGS_MAX_HISTORY == 64
    assert int(re.search(r"#define\s+PINN_LBFGS_RECORD_DOUBLES\s+(\d+)", header).group(1)) == _lib.PINN_LBFGS_RECORD_DOUBLES
    for key, idx in _lib.LBFGS_REC.items():
        macro = {"n_iter": "ITER", "h_diag": "HDIAG"}.get(key, key.upper())
        assert int(re.search(rf"#define\s+PINN_LBFGS_REC_{macro}\s+(\d+)", header).group(1)) == idx
    lib = _lib.load()
    assert lib.pinn_abi_version() == 2
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) > 0, name
    assert lib.pinn_lbfgs_direction.restype is ctypes.c_int and len(lib.pinn_lbfgs_direction.argtypes) == 12
    assert lib.pinn_lbfgs_eval_stats.restype is ctypes.c_int and len(lib.pinn_lbfgs_eval_stats.argtypes) == 7


def test_size_queries():
    lib = _lib.load()
    for h in (1, 5, 50, 64):
        s = h + 1
        assert lib.pinn_lbfgs_state_bytes(h) == 8 * (8 + s + 4 * s * s)
        assert lib.pinn_lbfgs_scratch_bytes(h) >= 8 * ((6 * h + 8) * 64 + 2 * h + 1)
        assert lib.pinn_lbfgs_scratch_bytes(h) >= 8 * 192  # what pinn_lbfgs_eval_stats needs
    for h in (0, -1, 65):
        assert lib.pinn_lbfgs_state_bytes(h) == 0 and lib.pinn_lbfgs_scratch_bytes(h) == 0


# ---------------------------------------------------------------------------------------------------------------------
# (b) the driver against torch.optim.LBFGS, both in double
# ---------------------------------------------------------------------------------------------------------------------
def _quadratic():
    lam = torch.logspace(0, 2, 50, dtype=torch.float64)  # condition 100
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(50, dtype=torch.float64, generator=g)
    return (lambda x: 0.5 * (lam * x * x).sum()), x0


def _rosenbrock():
    return (lambda x: (1 - x[0]) ** 2 + 100 * (x[1] - x[0] ** 2) ** 2), torch.tensor([-1.2, 1.0], dtype=torch.float64)


PROBLEMS = {"quadratic50": _quadratic, "rosenbrock": _rosenbrock}
KW = dict(max_iter=10, history_size=5, tolerance_grad=1e-7, tolerance_change=1e-9)


def _torch_run(f, x0, line_search_fn, steps=2):
    x = x0.clone().requires_grad_(True)
    opt = torch.optim.LBFGS([x], lr=1.0, line_search_fn=line_search_fn, **KW)

    def closure():
        opt.zero_grad()
        loss = f(x)
        loss.backward()
        return loss

    for _ in range(steps):
        opt.step(closure)
    return x.detach().clone(), opt.state[x]["func_evals"], opt.state[x]["n_iter"]


def _driver_run(f, x0, line_search_fn, steps=2):
    def fun(xn):
        x = torch.from_numpy(xn.copy()).requires_grad_(True)
        loss = f(x)
        (g,) = torch.autograd.grad(loss, x)
        return float(loss.detach()), g.numpy()

    backend = LM.ModelBackend(fun, x0.numpy(), KW["history_size"])
    drv = LBFGSDriver(backend, max_iter=KW["max_iter"], tolerance_grad=KW["tolerance_grad"],
                      tolerance_change=KW["tolerance_change"], line_search_fn=line_search_fn, lr=lambda: 1.0)
    for _ in range(steps):
        drv.step()
    assert backend.evals == drv.func_evals
    return torch.from_numpy(backend.x), drv.func_evals, drv.n_iter


@pytest.mark.parametrize("line_search_fn", ["strong_wolfe", None])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_driver_matches_torch_lbfgs(name, line_search_fn):
    """Two consecutive step() calls (history and state carried over).  The control comes first: torch's own evaluation
    count must not move under a 1e-12 relative change of theta_0, otherwise the count is not a property of the algorithm
    at this start and comparing it would test rounding."""
    f, x0 = PROBLEMS[name]()
    ref, evals, iters = _torch_run(f, x0, line_search_fn)
    _, evals_p, iters_p = _torch_run(f, x0 * (1 + 1e-12), line_search_fn)
    assert (evals, iters) == (evals_p, iters_p), "control: torch's own count moves under a 1e-12 perturbation of the start"
    got, d_evals, d_iters = _driver_run(f, x0, line_search_fn)
    err = float((got - ref).norm() / ref.norm())
    print(f"{name} {line_search_fn}: torch {evals} evaluations / {iters} iterations, driver {d_evals} / {d_iters}, theta rel {err:.2e}")
    assert (d_evals, d_iters) == (evals, iters)
    assert math.isfinite(err) and err <= 1e-8


def test_driver_stops_at_once_on_a_stationary_point():
    f, _ = _quadratic()
    x0 = torch.zeros(50, dtype=torch.float64)
    got, evals, iters = _driver_run(f, x0, "strong_wolfe", steps=1)
    assert (evals, iters) == (1, 0) and float(got.abs().max()) == 0.0


def test_model_ring_rejects_and_evicts():
    """The fp64 model's own semantics: a pair with y.s <= 1e-10 leaves the ring alone; a full ring drops its oldest pair."""
    rng = np.random.default_rng(0)
    lam = np.exp(rng.uniform(0, np.log(100.0), 7))
    m = LM.LBFGSModel(3)
    x = rng.standard_normal(7)
    m.direction(lam * x)
    firsts = []
    for k in range(5):
        x = x + 0.5 * m.d
        rec = m.direction(lam * x, 0.5)
        assert rec["accepted"] and rec["count"] == min(k + 1, 3)
        firsts.append(m.S[0].copy())
    assert not np.array_equal(firsts[2], firsts[3])  # wraparound: the oldest pair left
    S_before = [s.copy() for s in m.S]
    rec = m.direction(m.prev_grad.copy(), 0.5)  # y = 0: rejected
    assert not rec["accepted"] and rec["count"] == 3
    assert all(np.array_equal(a, b) for a, b in zip(S_before, m.S))
    d64 = LM.two_loop(m.prev_grad, m.S, m.Y, m.ro, m.h_diag)
    assert np.array_equal(d64, m.d)


# ---------------------------------------------------------------------------------------------------------------------
# (c) routing
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(kind, adaptive=False, history_size=10):
    cfg = Config.__new__(Config)
    cfg.device = torch.device("cpu")
    cfg.training = TrainingConfig(learning_rate=0.5, gradient_clipping=0.0, optimizer=kind,
                                  mode="forward")
    cfg.training.lbfgs.history_size = history_size
    if adaptive:
        cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy="rbw", alpha=0.7, eps=1e-6,
                                                              initial_weights=[0.3, 0.4, 0.3])
    return cfg


def _trainer(cfg, trainable=(), **kw):
    pde = P.BurgersEquation(P.PDEConfig(
        name="b", domain=[(-1.0, 1.0)], time_domain=(0.0, 1.0), parameters={"nu": 0.01 / math.pi},
        boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0}, exact_solution={}, dimension=1,
        device=torch.device("cpu"), training=cfg.training, trainable_parameters=list(trainable),
        parameter_initial_guesses={"nu": 0.02} if trainable else {}))
    return PDETrainer(torch.nn.Linear(2, 1), pde, {}, cfg, device=torch.device("cpu"), **kw)


@pytest.mark.parametrize("kind", ["lbfgs", "adam_lbfgs"])
def test_lbfgs_takes_the_launch_list_where_adam_does(kind):
    assert _trainer(_cfg("adam"))._manual_step_unsupported() is None
    assert _trainer(_cfg(kind))._manual_step_unsupported() is None
    assert _trainer(_cfg(kind, history_size=64))._manual_step_unsupported() is None


@pytest.mark.parametrize("kind", ["lbfgs", "adam_lbfgs"])
def test_refused_combinations_name_their_reason(kind):
    why = _trainer(_cfg(kind), trainable=["nu"])._manual_step_unsupported()
    assert why is not None and "trainable PDE coefficients" in why
    why = _trainer(_cfg(kind, adaptive=True))._manual_step_unsupported()
    assert why is not None and "adaptive loss weights" in why and "L-BFGS" in why
    why = _trainer(_cfg(kind, history_size=65))._manual_step_unsupported()
    assert why is not None and "history_size" in why
    tr = _trainer(_cfg(kind))
    tr.process_group = object()  # a process group cannot be built in this process; the routing only looks at its presence
    why = tr._manual_step_unsupported()
    assert why is not None and "process group" in why and "L-BFGS" in why
    reasons = {_trainer(_cfg(kind), trainable=["nu"])._manual_step_unsupported(),
               _trainer(_cfg(kind, adaptive=True))._manual_step_unsupported(),
               _trainer(_cfg(kind, history_size=65))._manual_step_unsupported(), why}
    assert len(reasons) == 4  # each its own


def test_graph_capture_still_refuses_lbfgs():
    for kind in ("lbfgs", "adam_lbfgs"):
        with pytest.raises(NotImplementedError, match="L-BFGS"):
            _trainer(_cfg(kind)).make_graphed_step(16)
