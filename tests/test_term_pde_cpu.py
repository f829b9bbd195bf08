"""Residuals given as data, without a GPU: (a) the fp64 model of `pinn_term_residual` (tests/term_pde_model.py) against
torch autograd of the same formula, and an fp32 evaluation in another order against the model's bound; (b) every
validation case of the entry point through the C ABI (all are answered before any HIP call), the declared and exported
symbols; (c) `TermPDE`: stream sets, constructor refusals, and what `PDETrainer._manual_step_unsupported()` says."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import pinnrl_amd  # noqa: F401
import term_pde_model as M
from pinnrl_amd import _lib
from pinnrl_amd import engine as E
from pinnrl_amd import pdes as P
from pinnrl_amd.config import AdaptiveWeightsConfig, Config, TrainingConfig
from pinnrl_amd.training import PDETrainer

FEATURE = (_lib.PinnTermPde, E.TermDesc, P.TermPDE)  # every test of this file, the model's included, belongs to the feature


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model
# ---------------------------------------------------------------------------------------------------------------------
def _torch_formula(nt, nx, terms, coef, jets, x, t):
    u = jets[0]
    v = {"u": u, "x": x, "t": t, "sin(u)": torch.sin(u), "cos(u)": torch.cos(u)}
    for name, k in M.T_ORDER.items():
        if k <= nt:
            v[name] = jets[k]
    for name, k in M.X_ORDER.items():
        if k <= nx:
            v[name] = jets[nt + k]
    r = torch.zeros_like(u)
    for c, factors in zip(coef, terms):
        p = torch.ones_like(u)
        for f in factors:
            p = p * v[f]
        r = r + c * p
    return r


def _torch_loss_sum(r, loss, delta):
    if loss == "mae":
        return r.abs().sum()
    if loss == "huber":
        return torch.nn.functional.huber_loss(r, torch.zeros_like(r), reduction="sum", delta=delta)
    return (r * r).sum()


@pytest.mark.parametrize("loss,delta", M.LOSSES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_model_matches_autograd_of_the_formula(name, loss, delta):
    nt, nx, terms, coef, jets, x, t, rbar = M.inputs(name, 37)
    gs = 0.37
    m = M.evaluate(nt, nx, terms, coef, jets, x, t, loss, delta, gs)
    J = torch.from_numpy(jets).double().requires_grad_(True)
    c = torch.from_numpy(coef).double().requires_grad_(True)
    r = _torch_formula(nt, nx, terms, c, J, torch.from_numpy(x).double(), torch.from_numpy(t).double())
    S = _torch_loss_sum(r, loss, delta)
    gJ, gc = torch.autograd.grad(gs * S, (J, c), retain_graph=True)
    np.testing.assert_allclose(m["r"], r.detach().numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(m["loss_sum"], float(S.detach()), rtol=1e-13)
    np.testing.assert_allclose(m["cot"], gJ.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(m["coef_sums"], gc.numpy(), rtol=1e-12, atol=1e-13)
    # the residual_cotangent form: <rbar, r> differentiated
    m2 = M.evaluate(nt, nx, terms, coef, jets, x, t, loss, delta, gs, residual_cotangent=rbar)
    gJ2, gc2 = torch.autograd.grad((torch.from_numpy(rbar).double() * r).sum(), (J, c))
    np.testing.assert_allclose(m2["cot"], gJ2.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(m2["coef_sums"], gc2.numpy(), rtol=1e-12, atol=1e-13)
    # dr/djet alone
    gJ3, = torch.autograd.grad(_torch_formula(nt, nx, terms, c.detach(), J, torch.from_numpy(x).double(),
                                              torch.from_numpy(t).double()).sum(), J)
    np.testing.assert_allclose(m["dr"], gJ3.numpy(), rtol=1e-12, atol=1e-13)


def _fp32_reversed(nt, nx, terms, coef, jets, x, t):
    """r and dr/djet in numpy fp32, terms and factors taken in reversed order, every summand added straight to its sum."""
    f32 = np.float32
    v = {"u": jets[0], "x": x, "t": t, "sin(u)": np.sin(jets[0]).astype(f32), "cos(u)": np.cos(jets[0]).astype(f32)}
    for name, k in M.T_ORDER.items():
        if k <= nt:
            v[name] = jets[k]
    for name, k in M.X_ORDER.items():
        if k <= nx:
            v[name] = jets[nt + k]
    N = jets.shape[1]
    r, dr = np.zeros(N, f32), np.zeros(jets.shape, f32)
    for c, factors in reversed(list(zip(coef, terms))):
        p = np.ones(N, f32)
        for f in reversed(factors):
            p = (p * v[f]).astype(f32)
        r = (r + (p * f32(c)).astype(f32)).astype(f32)
        for i in reversed(range(len(factors))):
            name = factors[i]
            if name in ("x", "t"):
                continue
            o = np.full(N, f32(c), f32)
            for g in reversed(range(len(factors))):
                if g != i:
                    o = (o * v[factors[g]]).astype(f32)
            if name == "sin(u)":
                s, o = 0, (o * v["cos(u)"]).astype(f32)
            elif name == "cos(u)":
                s, o = 0, (-(o * v["sin(u)"])).astype(f32)
            else:
                s = M.stream_of(name, nt, nx)
            dr[s] = (dr[s] + o).astype(f32)
    return r, dr


@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_fp32_evaluation_in_another_order_is_inside_the_bound(name):
    """The bound is not too tight: an fp32 evaluation that orders terms and factors the other way round, and adds the
    derivative summands without grouping them by term, stays inside it at every point."""
    nt, nx, terms, coef, jets, x, t, _ = M.inputs(name, 16421)
    m = M.evaluate(nt, nx, terms, coef, jets, x, t)
    r, dr = _fp32_reversed(nt, nx, terms, coef, jets, x, t)
    assert np.all(np.abs(r - m["r"]) <= m["r_bound"]), float(np.max(np.abs(r - m["r"]) / np.maximum(m["r_bound"], 1e-300)))
    assert np.all(np.abs(dr - m["dr"]) <= m["dr_bound"])
    # and it is a bound of fp32 size: relative to the absolute sums it is (T + F + 2) 2^-23
    T, F = len(terms), max(len(f) for f in terms)
    assert m["count"] == T + F + 2


@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_seeds_keep_the_kinks_of_the_loss_clear(name):
    """For mae and Huber the GPU test skips points whose fp64 |r| lies within its bound of 0 / delta.  The seeds of
    `term_pde_model.inputs` leave none there, on the model alone."""
    for N in M.SIZES:
        nt, nx, terms, coef, jets, x, t, _ = M.inputs(name, N)
        for loss, delta in M.LOSSES:
            m = M.evaluate(nt, nx, terms, coef, jets, x, t, loss, delta, 1.0 / N)
            assert int(m["unsafe"].sum()) == 0, (name, N, loss, int(m["unsafe"].sum()))


# ---------------------------------------------------------------------------------------------------------------------
# (b) the C ABI on the host
# ---------------------------------------------------------------------------------------------------------------------
def _desc(nt=1, nx=2, terms=(("u_t",), ("u", "u_x"), ("u_xx",))):
    d = _lib.PinnTermPde()
    d.time_order, d.space_order, d.n_terms, d.loss, d.huber_delta = nt, nx, len(terms), 0, 1.0
    for m, fs in enumerate(terms):
        d.terms[m].n_factors = len(fs)
        for f, name in enumerate(fs):
            d.terms[m].factor[f] = _lib.TERM_FACTOR[name]
    return d


def _call(d, coef=0x1000, jets=0x1000, x=None, t=None, N=8, scratch=None, loss_sum=None):
    """pinn_term_residual with made-up device addresses: every case below must be answered before any HIP call."""
    lib = _lib.load()
    return lib.pinn_term_residual(ctypes.byref(d), coef, jets, x, t, N, 1.0, None, None, loss_sum, None, None, scratch, None)


def test_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pinn_jet.h")).read()
    assert re.search(r"\bint pinn_term_residual\s*\(", hdr)
    assert "pinn_term_residual" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "pinn_term_residual")
    assert lib.pinn_abi_version() == 2 == _lib.PINN_ABI_VERSION
    for name, val in (("PINN_TERM_MAX_TERMS", 16), ("PINN_TERM_MAX_FACTORS", 4)):
        assert re.search(rf"#define {name} {val}\b", hdr) and getattr(_lib, name) == val
    assert _lib.PINN_TERM_SCRATCH_DOUBLES == 64 * 17 and "#define PINN_TERM_SCRATCH_DOUBLES (64 * (1 + PINN_TERM_MAX_TERMS))" in hdr
    # the factor enum of the header is the table of the binding, and the struct has the header's size
    codes = dict(re.findall(r"PINN_TERM_([A-Z_]+) = (\d+)", hdr))
    want = {"U": "u", "UT": "u_t", "UTT": "u_tt", "UX": "u_x", "UXX": "u_xx", "UXXX": "u_xxx", "UXXXX": "u_xxxx", "X": "x",
            "T": "t", "SIN_U": "sin(u)", "COS_U": "cos(u)"}
    assert {want[k]: int(v) for k, v in codes.items()} == _lib.TERM_FACTOR
    assert ctypes.sizeof(_lib.PinnTermPde) == 4 * (5 + 16 * 5)
    assert tuple(M.FACTORS) == tuple(sorted(_lib.TERM_FACTOR, key=_lib.TERM_FACTOR.get))


def test_validation_cases_are_answered_on_the_host():
    lib = _lib.load()
    BAD, MIS = -1, -3

    def err():
        return lib.pinn_last_error().decode()

    assert _call(_desc(), N=0) == 0  # N == 0: no-op, whatever the pointers
    assert _call(_desc(), N=0, jets=None, coef=None) == 0
    d = _desc()
    d.n_terms = 17
    assert _call(d) == BAD and "n_terms" in err()
    d.n_terms = -1
    assert _call(d) == BAD and "n_terms" in err()
    d = _desc()
    d.terms[1].n_factors = 5
    assert _call(d) == BAD and "n_factors" in err()
    d.terms[1].n_factors = -1
    assert _call(d) == BAD and "n_factors" in err()
    d = _desc()
    d.terms[0].factor[0] = 11
    assert _call(d) == BAD and "unknown factor" in err()
    d.terms[0].factor[0] = -1
    assert _call(d) == BAD and "unknown factor" in err()
    # a factor that names a stream the set does not hold
    for nt, nx, name in ((1, 2, "u_tt"), (1, 2, "u_xxx"), (0, 0, "u_t"), (2, 0, "u_x"), (1, 3, "u_xxxx")):
        assert _call(_desc(nt, nx, ((name,),))) == BAD and "does not hold" in err(), (nt, nx, name)
    # a stream set the library has no unit for
    for nt, nx in ((2, 1), (2, 3), (2, 4), (0, 1), (0, 2), (3, 0), (1, 5), (-1, 0)):
        assert _call(_desc(nt, nx, (("u",),))) == BAD and "not compiled" in err(), (nt, nx)
    for nt, nx in P.pde_base._STREAM_SETS:  # and every set it has one for passes that check
        assert _call(_desc(nt, nx, (("u",),)), N=0) == 0
    assert _call(_desc(), N=-1) == BAD and "N < 0" in err()
    assert _call(_desc(), jets=None) == BAD and "null" in err()
    assert _call(_desc(), coef=None) == BAD and "null" in err()
    assert _call(_desc(1, 2, (("x", "u"),)), x=None) == BAD and "X / T" in err()
    assert _call(_desc(1, 2, (("t",),)), x=0x1000, t=None) == BAD and "X / T" in err()
    assert _call(_desc(), scratch=0x1004, loss_sum=0x1000) == MIS and "8-byte" in err()
    assert _call(_desc(), scratch=None, loss_sum=0x1000) == BAD and "scratch" in err()
    assert lib.pinn_term_residual(None, 0x1000, 0x1000, None, None, 8, 1.0, None, None, None, None, None, None, None) == BAD


def test_engine_descriptor_object():
    cv = torch.tensor([1.0, 1.0, -0.1])
    td = E.TermDesc([("u_t",), ("u", "u_x"), ("u_xx",)], cv, 1, 2, "huber", 0.5)
    assert E.pde_streams(td) == (1, 2) and td.desc.n_terms == 3 and td.desc.loss == _lib.LOSS["huber"]
    assert [td.desc.terms[1].factor[f] for f in range(td.desc.terms[1].n_factors)] == [0, 3]
    l1 = td.with_loss("mae")
    assert l1.coef_values is cv and l1.desc.loss == _lib.LOSS["mae"] and l1.terms == td.terms
    with pytest.raises(ValueError, match="at most 16"):
        E.TermDesc([("u",)] * 17, torch.zeros(17), 1, 2)
    with pytest.raises(ValueError, match="at most 4"):
        E.TermDesc([("u",) * 5], torch.zeros(1), 1, 2)
    with pytest.raises(ValueError, match="unknown factor"):
        E.TermDesc([("u_y",)], torch.zeros(1), 1, 2)
    with pytest.raises(ValueError, match="coef_values"):
        E.TermDesc([("u",), ("u_t",)], torch.zeros(1), 1, 2)
    with pytest.raises(RuntimeError, match="ROCm device"):  # no CPU fallback
        E.term_residual(td, torch.zeros(4, 8), torch.zeros(8, 1), torch.zeros(8, 1))


# ---------------------------------------------------------------------------------------------------------------------
# (c) TermPDE and the trainer's routing
# ---------------------------------------------------------------------------------------------------------------------
def _config(training=None, dimension=1, trainable=(), parameters=None, observation=None):
    return P.PDEConfig(
        name="term", domain=[(-1.0, 1.0)] * dimension, time_domain=(0.0, 1.0), parameters=dict(parameters or {"nu": 0.02}),
        boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0}, exact_solution={}, dimension=dimension,
        device=torch.device("cpu"), training=training, trainable_parameters=list(trainable),
        parameter_initial_guesses={"nu": 0.05} if trainable else {}, observation_data=observation)


BURGERS = [(1.0, ("u_t",)), (1.0, ("u", "u_x")), ((-1.0, "nu"), ("u_xx",))]


def test_term_pde_picks_the_smallest_covering_stream_set():
    cases = {
        (("u",),): (0, 0), (("u_t",),): (1, 0), (("u_t",), ("u_x",)): (1, 1), (("u_t",), ("u", "u_x"), ("u_xx",)): (1, 2),
        (("u_t",), ("u", "u_x"), ("u_xxx",)): (1, 3), (("u_t",), ("u_xxxx",)): (1, 4), (("u_tt",), ("sin(u)",)): (2, 0),
        (("u_tt",), ("u_xx",)): (2, 2), (("u_tt",), ("u_x",)): (2, 2), (("u_xx",),): (1, 2), (("x", "t"), ()): (0, 0),
    }
    for factors, want in cases.items():
        pde = P.TermPDE(_config(), [(1.0, f) for f in factors])
        assert (pde._nt, pde._nx) == want, (factors, (pde._nt, pde._nx))
        assert E.pde_streams(pde._pde_desc()) == want
    pde = P.TermPDE(_config(), BURGERS)
    assert isinstance(pde, P.PDEBase) and "TermPDE" in P.__dict__ and P.TermPDE not in P._BY_TYPE.values()
    td = pde._pde_desc()
    assert td is pde._pde_desc() and td.coef_values is pde.coef_values  # persistent: nothing is rebuilt inside a step
    assert td.coef_values.tolist() == pytest.approx([1.0, 1.0, -0.02])
    assert pde._pde_desc_l1().coef_values is td.coef_values and pde._pde_desc_l1().desc.loss == _lib.LOSS["mae"]
    with pytest.raises(NotImplementedError, match="exact_solution_fn"):
        pde.exact_solution(torch.zeros(2, 1), torch.zeros(2, 1))
    pde = P.TermPDE(_config(), BURGERS, exact_solution_fn=lambda x, t: x + 2 * t)
    assert pde.exact_solution(torch.ones(2, 1), torch.ones(2, 1)).tolist() == [[3.0], [3.0]]


def test_term_pde_constructor_refusals():
    with pytest.raises(NotImplementedError, match="no compiled stream set"):
        P.TermPDE(_config(), [(1.0, ("u_tt",)), (1.0, ("u_xxx",))])
    with pytest.raises(NotImplementedError, match="no compiled stream set"):
        P.TermPDE(_config(), [(1.0, ("u_tt", "u_xxxx"))])
    with pytest.raises(NotImplementedError, match="dimension 2"):
        P.TermPDE(_config(dimension=2), BURGERS)
    with pytest.raises(ValueError, match="at most 16"):
        P.TermPDE(_config(), [(1.0, ("u",))] * 17)
    with pytest.raises(ValueError, match="at most 4"):
        P.TermPDE(_config(), [(1.0, ("u",) * 5)])
    with pytest.raises(ValueError, match="unknown factor"):
        P.TermPDE(_config(), [(1.0, ("u_xt",))])
    with pytest.raises(ValueError, match="not in config.parameters"):
        P.TermPDE(_config(), [((1.0, "kappa"), ("u",))])
    P.TermPDE(_config(), [(1.0, ("u",))] * 16)  # the limits themselves are fine
    P.TermPDE(_config(), [(1.0, ("u",) * 4)])


def test_trainable_coefficients_stay_in_the_torch_formula():
    """`_residual_from_jets` is the model's formula, and a trainable named parameter is live in it."""
    nt, nx, terms, coef, jets, x, t, _ = M.inputs("sixteen", 37)
    pde = P.TermPDE(_config(), [(float(c), f) for c, f in zip(coef, terms)])
    r = pde._residual_from_jets(torch.from_numpy(jets).double(), torch.from_numpy(x).double(), nt, nx, torch.from_numpy(t).double())
    np.testing.assert_allclose(r.numpy(), M.evaluate(nt, nx, terms, coef, jets, x, t)["r"], rtol=1e-12, atol=1e-12)
    pde = P.TermPDE(_config(trainable=["nu"]), BURGERS)
    assert pde._has_trainable_coefficients() and not P.TermPDE(_config(), BURGERS)._has_trainable_coefficients()
    J = torch.randn(4, 5)
    r = pde._residual_from_jets(J, torch.zeros(5), 1, 2, torch.zeros(5))
    g, = torch.autograd.grad(r.sum(), pde._trainable_params["nu"])
    assert float(g) == pytest.approx(float(-J[3].sum()))


def _cfg(kind="adam", adaptive=None, mode="forward"):
    cfg = Config.__new__(Config)
    cfg.device = torch.device("cpu")
    cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, optimizer=kind, mode=mode)
    if adaptive:
        cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy=adaptive, alpha=0.7, eps=1e-6)
    return cfg


def _trainer(cfg, **kw):
    pde = P.TermPDE(_config(training=cfg.training, **kw), BURGERS)
    return PDETrainer(torch.nn.Linear(2, 1), pde, {}, cfg, device=torch.device("cpu"))


@pytest.mark.parametrize("kind,adaptive", [("adam", None), ("lbfgs", None), ("adam_lbfgs", None), ("adam", "rbw"), ("adam", "lrw")])
def test_forward_mode_takes_the_launch_list(kind, adaptive):
    assert _trainer(_cfg(kind, adaptive))._manual_step_unsupported() is None


def test_refused_combinations_name_their_reason():
    why_coef = _trainer(_cfg(), trainable=["nu"])._manual_step_unsupported()
    assert why_coef is not None and "TermPDE" in why_coef and "trainable term coefficients" in why_coef
    obs = {"x": [0.0, 0.5], "t": [0.1, 0.2], "u": [0.0, 0.1]}
    why_data = _trainer(_cfg(mode="data_augmented"), observation=obs)._manual_step_unsupported()
    assert why_data is not None and "TermPDE" in why_data and "data mode" in why_data
    tr = _trainer(_cfg())
    tr.process_group = object()  # a process group cannot be built in this process; the routing only looks at its presence
    why_pg = tr._manual_step_unsupported()
    assert why_pg is not None and "TermPDE" in why_pg and "process group" in why_pg
    assert len({why_coef, why_data, why_pg}) == 3  # each its own
    # a trainable parameter that no term names is not a term coefficient: the general reason for such parameters applies
    pde = P.TermPDE(_config(training=_cfg().training, trainable=["nu"]), [(1.0, ("u_t",)), (1.0, ("u", "u_x"))])
    assert not pde._has_trainable_coefficients()
    why = PDETrainer(torch.nn.Linear(2, 1), pde, {}, _cfg(), device=torch.device("cpu"))._manual_step_unsupported()
    assert why is not None and "term coefficients" not in why and "trainable parameters" in why


def test_coefficient_tensor_is_persistent_whatever_the_spelling_of_the_device():
    """The tensor is rebuilt only when the REQUESTED device changes; the comparison never involves the device a tensor
    reports (a tensor made on torch.device("cuda") reports cuda:0, which is not equal to the request)."""
    pde = P.TermPDE(_config(), BURGERS)
    cv = pde.coef_values
    assert pde.coef_values is cv and pde._coef_device == torch.device("cpu")
    pde._coef_device = torch.device("meta")  # stands for a request the tensor does not report back
    pde.device = torch.device("meta")
    pde._coef_values = cv
    assert pde.coef_values is cv  # requested == requested: kept, although cv.device is cpu
    pde.device = torch.device("cpu")
    assert pde.coef_values is not cv  # a changed request rebuilds
