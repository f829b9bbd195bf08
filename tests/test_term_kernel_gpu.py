"""`pinn_term_residual` against its fp64 model (tests/term_pde_model.py) on synthetic standard-normal jets with O(1)
coefficients: six programs on their stream sets x four sizes (1, 37, 1027 = several blocks and a ragged last one, 16 421 =
past 64 x 256, where the grid-stride loop runs twice) x the three loss kinds.

Per point, r and the cotangents are within the model's bound; the loss sum and the coefficient sums (double accumulation of
fp32 summands) within 1e-6 of the sum of the absolute summands.  Outputs are poisoned with NaN and carry guard rows that
must stay NaN; two runs are bit-identical; the `residual_cotangent` form and the one-launch residual-only form have their
own checks.  For mae and Huber, points whose fp64 |r| lies within its bound of 0 / delta may take the other branch of l'
on the device: they are skipped, fewer than 1 % of them (tests/test_term_pde_cpu.py shows on the model alone that the seeds
leave none)."""

import ctypes

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import term_pde_model as M
from pinnrl_amd import _lib
from pinnrl_amd import engine as E

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-6
GUARD = 64  # floats of NaN after every output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


_cache = {}


def _case(name, N, dev):
    """Inputs on the host and on the device, computed once per (program, size) and left unchanged."""
    key = (name, N)
    if key not in _cache:
        nt, nx, terms, coef, jets, x, t, rbar = M.inputs(name, N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("jets", jets), ("x", x), ("t", t), ("rbar", rbar))}
        _cache[key] = (nt, nx, terms, coef, jets, x, t, rbar, d)
    return _cache[key]


def _poisoned(n, dev):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def _run(td, d, N, K, dev, grad_scale, rbar=None, want=("r", "loss", "cot", "coef"), loss0=0.0, coef0=0.0):
    """One raw call through the C ABI with poisoned, guarded outputs.  Returns host arrays and the guards."""
    lib = _lib.load()
    T = td.desc.n_terms
    r = _poisoned(N, dev) if "r" in want else None
    cot = _poisoned(K * N, dev) if "cot" in want else None
    loss = torch.full((1 + GUARD,), float("nan"), dtype=torch.float32, device=dev) if "loss" in want else None
    cg = torch.full((16 + GUARD,), float("nan"), dtype=torch.float32, device=dev) if "coef" in want else None
    if loss is not None:
        loss[0] = loss0
    if cg is not None:
        cg[:T] = coef0
    scratch = torch.full((_lib.PINN_TERM_SCRATCH_DOUBLES + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    opt = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        rc = lib.pinn_term_residual(ctypes.byref(td.desc), d["coef"].data_ptr(), d["jets"].data_ptr(), d["x"].data_ptr(),
                                    d["t"].data_ptr(), N, float(grad_scale), opt(rbar), opt(r), opt(loss), opt(cot), opt(cg),
                                    scratch.data_ptr() if ("loss" in want or "coef" in want) else None,
                                    torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc)
    torch.cuda.synchronize(dev)
    out = {}
    for k, v, n in (("r", r, N), ("cot", cot, K * N), ("loss", loss, 1), ("coef", cg, T)):
        if v is not None:
            h = v.cpu().numpy()
            out[k] = h[:n].copy()
            assert np.all(np.isnan(h[n:])), f"{k}: written past its {n} floats"
    assert np.all(np.isnan(scratch[_lib.PINN_TERM_SCRATCH_DOUBLES:].cpu().numpy())), "scratch: written past PINN_TERM_SCRATCH_DOUBLES"
    return out


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_kernel_matches_the_model(name, N, dev):
    nt, nx, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    K, T = 1 + nt + nx, len(terms)
    gs = 1.0 / N
    for loss, delta in M.LOSSES:
        td = E.TermDesc(terms, d["coef"], nt, nx, loss, delta)
        m = M.evaluate(nt, nx, terms, coef, jets, x, t, loss, delta, gs)
        o = _run(td, d, N, K, dev, gs, loss0=0.25, coef0=-0.5)
        ok = ~m["unsafe"]
        skipped = int(m["unsafe"].sum())
        print(f"{name} N={N} {loss}: skipped {skipped}")
        assert skipped < 0.01 * N
        # residual: every point, whatever the loss
        e_r = np.abs(o["r"] - m["r"])
        print(f"  r: max err / bound = {float(np.max(e_r / np.maximum(m['r_bound'], 1e-300))):.3f}")
        assert not np.any(np.isnan(o["r"])) and np.all(e_r <= m["r_bound"])
        # cotangents: every stream of every point is written; the bound holds away from the kinks
        cot = o["cot"].reshape(K, N)
        assert not np.any(np.isnan(cot))
        e_c = np.abs(cot - m["cot"])[:, ok]
        print(f"  cot: max err / bound = {float(np.max(e_c / np.maximum(m['cot_bound'][:, ok], 1e-300))):.3f}")
        assert np.all(e_c <= m["cot_bound"][:, ok])
        # sums: += into what was there
        e_l = abs(float(o["loss"][0]) - (0.25 + m["loss_sum"]))
        print(f"  loss sum: err / abs sum = {e_l / max(m['loss_abs'], 1e-300):.2e}")
        assert e_l <= SUM_TOL * (0.25 + m["loss_abs"])
        # a point on the wrong side of a kink changes its rbar by at most 2 |grad_scale| l'-range: allowed for, zero when none is skipped
        slack = 2.0 * abs(gs) * max(delta, 1.0) * np.abs(m["coef_prod"][:, ~ok]).sum(1)
        e_g = np.abs(o["coef"].astype(np.float64) - (-0.5 + m["coef_sums"]))
        print(f"  coef sums: max err / abs sum = {float(np.max(e_g / np.maximum(m['coef_abs'], 1e-300))):.2e}")
        assert np.all(e_g <= SUM_TOL * (0.5 + m["coef_abs"]) + slack)
        # bit-identical across runs
        o2 = _run(td, d, N, K, dev, gs, loss0=0.25, coef0=-0.5)
        for k in o:
            assert np.array_equal(o[k].view(np.uint32), o2[k].view(np.uint32)), f"{k} differs between two runs"


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_cotangent_form(name, N, dev):
    """A given cotangent replaces grad_scale l'(r): the loss kind and grad_scale no longer reach the cotangents."""
    nt, nx, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    K = 1 + nt + nx
    td = E.TermDesc(terms, d["coef"], nt, nx, "mae", 1.0)
    m = M.evaluate(nt, nx, terms, coef, jets, x, t, "mae", 1.0, 123.0, residual_cotangent=rbar)
    o = _run(td, d, N, K, dev, 123.0, rbar=d["rbar"], want=("cot", "coef"))
    cot = o["cot"].reshape(K, N)
    assert np.all(np.abs(cot - m["cot"]) <= m["cot_bound"])
    assert np.all(np.abs(o["coef"] - m["coef_sums"]) <= SUM_TOL * m["coef_abs"])
    # through the engine wrapper, cotangents only: one launch
    _, cot2 = E.term_residual(td, d["jets"], d["x"], d["t"], residual_cotangent=d["rbar"], want_residual=False, want_cotangents=True)
    assert np.array_equal(cot2.cpu().numpy().view(np.uint32), cot.view(np.uint32))


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_only_form(name, N, dev):
    """No loss, no cotangents, no coefficient sums: one launch that needs no scratch, the same residual bit for bit."""
    nt, nx, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    K = 1 + nt + nx
    td = E.TermDesc(terms, d["coef"], nt, nx)
    m = M.evaluate(nt, nx, terms, coef, jets, x, t)
    o = _run(td, d, N, K, dev, 0.0, want=("r",))
    assert np.all(np.abs(o["r"] - m["r"]) <= m["r_bound"])
    full = _run(td, d, N, K, dev, 1.0 / N)
    assert np.array_equal(o["r"].view(np.uint32), full["r"].view(np.uint32))
    r, cot = E.term_residual(td, d["jets"], d["x"], d["t"])
    assert cot is None and r.shape == (N, 1) and np.array_equal(r.cpu().numpy().reshape(-1).view(np.uint32), o["r"].view(np.uint32))


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_coefficient_sums_without_cotangents(name, N, dev):
    """coef_grads with a null jet_cotangents (and a null residual): the sums alone, the same bits as in the full call."""
    nt, nx, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    K = 1 + nt + nx
    gs = 1.0 / N
    td = E.TermDesc(terms, d["coef"], nt, nx, "mse", 1.0)
    m = M.evaluate(nt, nx, terms, coef, jets, x, t, "mse", 1.0, gs)
    o = _run(td, d, N, K, dev, gs, want=("coef",), coef0=-0.5)
    e_g = np.abs(o["coef"].astype(np.float64) - (-0.5 + m["coef_sums"]))
    assert np.all(e_g <= SUM_TOL * (0.5 + m["coef_abs"]))
    full = _run(td, d, N, K, dev, gs, loss0=0.25, coef0=-0.5)
    assert np.array_equal(o["coef"].view(np.uint32), full["coef"].view(np.uint32))
    # and the loss sum alone
    o = _run(td, d, N, K, dev, gs, want=("loss",), loss0=0.25)
    assert np.array_equal(o["loss"].view(np.uint32), full["loss"].view(np.uint32))


def test_coefficients_are_read_at_launch_time(dev):
    nt, nx, terms, coef, jets, x, t, rbar, d = _case("burgers", 1027, dev)
    cv = d["coef"].clone()
    td = E.TermDesc(terms, cv, nt, nx)
    r0, _ = E.term_residual(td, d["jets"], d["x"], d["t"])
    cv[2] = -0.5
    r1, _ = E.term_residual(td, d["jets"], d["x"], d["t"])
    c2 = coef.copy()
    c2[2] = -0.5
    m = M.evaluate(nt, nx, terms, c2, jets, x, t)
    assert np.all(np.abs(r1.cpu().numpy().reshape(-1) - m["r"]) <= m["r_bound"])
    assert not torch.equal(r0, r1)
