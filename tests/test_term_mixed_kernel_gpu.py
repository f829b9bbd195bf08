"""`pinn_term_residual_mixed` against its fp64 model (tests/term_mixed_model.py) on synthetic standard-normal blocks with
O(1) coefficients: u_xy alone, u_xx u_yy - u_xy u_xy, the 2-D bi-Laplacian, a 3-D program with all three pairs, a bi-Laplacian
in (y, z), one with sin(u), coordinate factors and repeated derived factors x four sizes (1, 255, 257 = one block ragged and a
second one, 64 x 256 + 1 = past the fixed grid, where the grid-stride loop takes a second trip) x the three loss kinds.

Per point, r and the cotangents of every block are within the model's bound; every cotangent row the program never reads
(row 0 of the blocks >= 1, rows 0, 1 and 3 of a P block, rows 0 .. 3 of a Q block) is exactly zero; the loss sum and the
coefficient sums (double accumulation of fp32 summands) within 1e-6 of the sum of the absolute summands, plus what the errors
of the derived factors move.  Outputs are poisoned with NaN and carry guard rows that must stay NaN; two runs are
bit-identical; the `residual_cotangent` form and the one-launch residual-only form have their own checks.  For mae and Huber,
points whose fp64 |r| lies within its bound of 0 / delta may take the other branch of l' on the device: they are skipped
(tests/test_term_mixed_cpu.py shows on the model alone that the seeds leave none)."""

import ctypes

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import term_mixed_model as M
from pinnrl_amd import _lib
from pinnrl_amd import engine as E

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-6
GUARD = 64  # floats of NaN after every output
NB = M.BLOCKS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


_cache = {}


def _case(name, N, dev):
    """Inputs on the host and on the device, computed once per (program, size) and left unchanged."""
    key = (name, N)
    if key not in _cache:
        dim, nt, nx, pair, terms, coef, jets, x, t, rbar = M.inputs(name, N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar))}
        d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
        _cache[key] = (dim, nt, nx, pair, terms, coef, jets, x, t, rbar, d)
    return _cache[key]


_models = {}


def _model(name, N, loss, delta, gs, rbar=None):
    """The fp64 reference, computed once per case and shared."""
    key = (name, N, loss, delta, gs, rbar is not None)
    if key not in _models:
        dim, nt, nx, pair, terms, coef, jets, x, t, rb = M.inputs(name, N)
        _models[key] = M.evaluate(dim, nt, nx, pair, terms, coef, jets, x, t, loss, delta, gs, residual_cotangent=rb if rbar is not None else None)
    return _models[key]


def _poisoned(n, dev):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def _run(td, d, N, dev, grad_scale, rbar=None, want=("r", "loss", "cot", "coef"), loss0=0.0, coef0=0.0):
    """One raw call through the C ABI with poisoned, guarded outputs.  Returns host arrays (cot: a list of blocks)."""
    lib = _lib.load()
    T = td.desc.n_terms
    rows = [None if j is None else j.shape[0] for j in d["jets"]]
    r = _poisoned(N, dev) if "r" in want else None
    cot = [None if k is None else _poisoned(k * N, dev) for k in rows] if "cot" in want else None
    loss = torch.full((1 + GUARD,), float("nan"), dtype=torch.float32, device=dev) if "loss" in want else None
    cg = torch.full((16 + GUARD,), float("nan"), dtype=torch.float32, device=dev) if "coef" in want else None
    if loss is not None:
        loss[0] = loss0
    if cg is not None:
        cg[:T] = coef0
    scratch = torch.full((_lib.PINN_TERM_SCRATCH_DOUBLES + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    opt = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
    jptr = (ctypes.c_void_p * NB)(*[opt(j) for j in d["jets"]])
    cptr = (ctypes.c_void_p * NB)(*[opt(c) for c in cot]) if cot is not None else None
    with torch.cuda.device(dev):
        rc = lib.pinn_term_residual_mixed(ctypes.byref(td.desc), d["coef"].data_ptr(), jptr, d["x"].data_ptr(), d["t"].data_ptr(), N,
                                          float(grad_scale), opt(rbar), opt(r), opt(loss), cptr, opt(cg),
                                          scratch.data_ptr() if ("loss" in want or "coef" in want) else None,
                                          torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc)
    torch.cuda.synchronize(dev)
    out = {}
    for k, v, n in (("r", r, N), ("loss", loss, 1), ("coef", cg, T)):
        if v is not None:
            h = v.cpu().numpy()
            out[k] = h[:n].copy()
            assert np.all(np.isnan(h[n:])), f"{k}: written past its {n} floats"
    if cot is not None:
        out["cot"] = []
        for b, (c, k) in enumerate(zip(cot, rows)):
            if c is None:
                out["cot"].append(None)
                continue
            h = c.cpu().numpy()
            assert np.all(np.isnan(h[k * N:])), f"cotangent block {b}: written past its {k} x {N} floats"
            out["cot"].append(h[: k * N].reshape(k, N).copy())
    assert np.all(np.isnan(scratch[_lib.PINN_TERM_SCRATCH_DOUBLES:].cpu().numpy())), "scratch: written past PINN_TERM_SCRATCH_DOUBLES"
    return out


def _same_bits(a, b):
    if isinstance(a, list):
        return all((x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _unread_rows(b, rows):
    if b == 0:
        return []
    if b < 3:
        return [0]
    return [s for s in range(rows) if not (s == 4 or (s == 2 and b < 6))]


def _check_cot(o, m, ok, label):
    for b in range(NB):
        if m["cot"][b] is None:
            assert o["cot"][b] is None
            continue
        cot = o["cot"][b]
        assert not np.any(np.isnan(cot)), f"{label}: block {b} holds an unwritten value"
        for s in _unread_rows(b, cot.shape[0]):
            assert not np.any(cot[s]), f"{label}: row {s} of block {b} is not zero"
        e = np.abs(cot - m["cot"][b])[:, ok]
        bd = m["cot_bound"][b][:, ok]
        print(f"  {label} block {b}: max err / bound = {float(np.max(e / np.maximum(bd, 1e-300))) if e.size else 0.0:.3f}")
        assert np.all(e <= bd), (label, b)


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_kernel_matches_the_model(name, N, dev):
    dim, nt, nx, pair, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    gs = 1.0 / N
    for loss, delta in M.LOSSES:
        td = E.MixedTermDesc(terms, d["coef"], dim, nt, nx, pair, loss, delta)
        m = _model(name, N, loss, delta, gs)
        o = _run(td, d, N, dev, gs, loss0=0.25, coef0=-0.5)
        ok = ~m["unsafe"]
        skipped = int(m["unsafe"].sum())
        print(f"{name} N={N} {loss}: skipped {skipped}")
        assert skipped <= 0.01 * N
        e_r = np.abs(o["r"] - m["r"])
        print(f"  r: max err / bound = {float(np.max(e_r / np.maximum(m['r_bound'], 1e-300))):.3f}")
        assert not np.any(np.isnan(o["r"])) and np.all(e_r <= m["r_bound"])
        _check_cot(o, m, ok, "cot")
        e_l = abs(float(o["loss"][0]) - (0.25 + m["loss_sum"]))
        print(f"  loss sum: err / abs sum = {e_l / max(m['loss_abs'], 1e-300):.2e}")
        assert e_l <= SUM_TOL * (0.25 + m["loss_abs"])
        # a point on the wrong side of a kink changes its rbar by at most 2 |grad_scale| l'-range: zero when none is skipped
        slack = 2.0 * abs(gs) * max(delta, 1.0) * np.abs(m["coef_prod"][:, ~ok]).sum(1)
        e_g = np.abs(o["coef"].astype(np.float64) - (-0.5 + m["coef_sums"]))
        print(f"  coef sums: max err / abs sum = {float(np.max(e_g / np.maximum(m['coef_abs'], 1e-300))):.2e}")
        assert np.all(e_g <= SUM_TOL * (0.5 + m["coef_abs"]) + m["coef_in"] + slack)
        o2 = _run(td, d, N, dev, gs, loss0=0.25, coef0=-0.5)  # bit-identical across runs
        for k in o:
            assert _same_bits(o[k], o2[k]), f"{k} differs between two runs"


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_cotangent_form(name, N, dev):
    """A given cotangent replaces grad_scale l'(r): the loss kind and grad_scale no longer reach the cotangents."""
    dim, nt, nx, pair, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    td = E.MixedTermDesc(terms, d["coef"], dim, nt, nx, pair, "mae", 1.0)
    m = _model(name, N, "mae", 1.0, 123.0, rbar=rbar)
    o = _run(td, d, N, dev, 123.0, rbar=d["rbar"], want=("cot", "coef"))
    _check_cot(o, m, np.ones(N, dtype=bool), "cot (given rbar)")
    assert np.all(np.abs(o["coef"] - m["coef_sums"]) <= SUM_TOL * m["coef_abs"] + m["coef_in"])
    # through the engine wrapper, cotangents only: one launch, the same bits
    _, cot2 = E.term_residual_mixed(td, d["jets"], d["x"], d["t"], residual_cotangent=d["rbar"], want_residual=False, want_cotangents=True)
    assert _same_bits([None if c is None else c.cpu().numpy() for c in cot2], o["cot"])


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_only_and_sums_only_forms(name, N, dev):
    """No loss, no cotangents, no coefficient sums: one launch that needs no scratch, the same residual bit for bit; and the
    sums without the cotangent table: the same bits as in the full call."""
    dim, nt, nx, pair, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    gs = 1.0 / N
    td = E.MixedTermDesc(terms, d["coef"], dim, nt, nx, pair)
    m = _model(name, N, "mse", 1.0, gs)
    o = _run(td, d, N, dev, 0.0, want=("r",))
    assert np.all(np.abs(o["r"] - m["r"]) <= m["r_bound"])
    full = _run(td, d, N, dev, gs, loss0=0.25, coef0=-0.5)
    assert _same_bits(o["r"], full["r"])
    r, cot = E.term_residual_mixed(td, d["jets"], d["x"], d["t"])
    assert cot is None and r.shape == (N, 1) and _same_bits(r.cpu().numpy().reshape(-1), o["r"])
    o = _run(td, d, N, dev, gs, want=("coef",), coef0=-0.5)
    assert _same_bits(o["coef"], full["coef"])
    o = _run(td, d, N, dev, gs, want=("loss",), loss0=0.25)
    assert _same_bits(o["loss"], full["loss"])


def test_coefficients_are_read_at_launch_time(dev):
    dim, nt, nx, pair, terms, coef, jets, x, t, rbar, d = _case("monge_ampere", 257, dev)
    cv = d["coef"].clone()
    td = E.MixedTermDesc(terms, cv, dim, nt, nx, pair)
    r0, _ = E.term_residual_mixed(td, d["jets"], d["x"], d["t"])
    cv[1] = -0.5
    r1, _ = E.term_residual_mixed(td, d["jets"], d["x"], d["t"])
    c2 = coef.copy()
    c2[1] = -0.5
    m = M.evaluate(dim, nt, nx, pair, terms, c2, jets, x, t)
    assert np.all(np.abs(r1.cpu().numpy().reshape(-1) - m["r"]) <= m["r_bound"])
    assert not torch.equal(r0, r1)
