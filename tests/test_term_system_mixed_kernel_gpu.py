"""`pinn_term_residual_system_mixed` against its fp64 model (tests/term_system_mixed_model.py) on synthetic standard-normal blocks
with O(1) coefficients: five programs — (a) 2-D elasticity (C = E = 2, each field naming the other's u_xy), (b) 3-D elasticity
(C = E = 3, all three pairs, each field naming two), (c) the caps at the LDS maximum (C = E = 4, dimension 3, 32 terms, every
field naming all three pairs, trig and coordinate factors, the same mixed factor twice in one term), (d) one pair of one field
(every other P block NULL, a field no term names), (e) the sibling's Navier-Stokes with all pair orders 0 — x the sibling's five
sizes (1, 255, 256, 257 = one block ragged and a second one, 64 x 256 + 3 = a second grid-stride round) x the three loss kinds,
with and without `residual_cotangent`, `coef_grads` and `eq_loss_sums`.

Per point, the residual of every equation and every cotangent row of all 6 C blocks are within the model's bound; the rows the
model marks untouched (rows 0 and 1 of every P block, row 0 of every axis block with a >= 1, every block of the unnamed field)
are exactly zero; the weighted loss sum, the per-equation sums and the coefficient sums within 1e-6 of the sum of the absolute
summands.  Outputs are poisoned with NaN and carry guard floats that must stay NaN; two calls are bit-identical.  On (e) the
residuals and cotangent blocks are bit-identical to `pinn_term_residual_system` on the same inputs.  For mae and Huber, points
whose fp64 |r_e| lies within its bound of 0 / delta may take the other branch of l' on the device: they are skipped
(tests/test_term_system_mixed_cpu.py shows on the model alone that the seeds leave at most 1 %)."""

import ctypes

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import term_system_mixed_model as M
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
        dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar = M.inputs(name, N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar))}
        d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
        _cache[key] = (dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, d)
    return _cache[key]


def _desc(name, d, loss="mse", delta=1.0):
    dim, nt, nx, pair, n_eq, terms, _ = M.PROGRAMS[name]
    factors, eq_of = M.engine_terms(terms)
    return E.MixedSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, M.EQ_WEIGHTS[name], loss, delta)


def _poisoned(n, dev):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def _run(td, d, N, dev, grad_scale, rbar=None, want=("r", "loss", "eq", "cot", "coef"), loss0=0.0, eq0=0.0, coef0=0.0, entry=None):
    """One raw call through the C ABI with poisoned, guarded outputs.  Returns host arrays (cot: a list of blocks)."""
    lib = _lib.load()
    T, Eq = td.desc.n_terms, td.n_equations
    rows = [None if j is None else j.shape[0] for j in d["jets"]]
    nb = len(rows)  # 6 C (3 C for the sibling's entry point)
    r = _poisoned(Eq * N, dev) if "r" in want else None
    cot = [None if k is None else _poisoned(k * N, dev) for k in rows] if "cot" in want else None
    loss = _poisoned(1, dev) if "loss" in want else None
    eq = _poisoned(Eq, dev) if "eq" in want else None
    cg = _poisoned(_lib.PINN_SYSTEM_MAX_TERMS, dev) if "coef" in want else None
    if loss is not None:
        loss[0] = loss0
    if eq is not None:
        eq[:Eq] = eq0
    if cg is not None:
        cg[:T] = coef0
    scratch = torch.full((_lib.PINN_SYSTEM_SCRATCH_DOUBLES + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    opt = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
    jptr = (ctypes.c_void_p * nb)(*[opt(j) for j in d["jets"]])
    cptr = (ctypes.c_void_p * nb)(*[opt(c) for c in cot]) if cot is not None else None
    sums = any(k in want for k in ("loss", "eq", "coef"))
    with torch.cuda.device(dev):
        rc = (entry or lib.pinn_term_residual_system_mixed)(ctypes.byref(td.desc), d["coef"].data_ptr(), jptr, d["x"].data_ptr(), d["t"].data_ptr(), N,
                                           float(grad_scale), opt(rbar), opt(r), opt(loss), opt(eq), cptr, opt(cg),
                                           scratch.data_ptr() if sums else None, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc)
    torch.cuda.synchronize(dev)
    out = {}
    for k, v, n in (("r", r, Eq * N), ("loss", loss, 1), ("eq", eq, Eq), ("coef", cg, T)):
        if v is not None:
            h = v.cpu().numpy()
            out[k] = h[:n].copy()
            assert np.all(np.isnan(h[n:])), f"{k}: written past its {n} floats"
    if "r" in out:
        out["r"] = out["r"].reshape(Eq, N)
    if cot is not None:
        out["cot"] = []
        for b, (c, k) in enumerate(zip(cot, rows)):
            if c is None:
                out["cot"].append(None)
                continue
            h = c.cpu().numpy()
            assert np.all(np.isnan(h[k * N:])), f"cotangent block {b}: written past its {k} x {N} floats"
            out["cot"].append(h[: k * N].reshape(k, N).copy())
    assert np.all(np.isnan(scratch[_lib.PINN_SYSTEM_SCRATCH_DOUBLES:].cpu().numpy())), "scratch: written past PINN_SYSTEM_SCRATCH_DOUBLES"
    return out


def _same_bits(a, b):
    if isinstance(a, list):
        return all((x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_cot(o, m, ok, label):
    worst = 0.0
    for b, want in enumerate(m["cot"]):
        if want is None:
            assert o["cot"][b] is None
            continue
        cot = o["cot"][b]
        assert not np.any(np.isnan(cot)), f"{label}: block {b} holds an unwritten value"
        for row in range(cot.shape[0]):
            if not m["touched"][b][row]:
                assert not np.any(cot[row]), f"{label}: row {row} of block {b} of {len(m['cot'])} is not zero"
        e = np.abs(cot - want)[:, ok]
        bd = m["cot_bound"][b][:, ok]
        if e.size:
            worst = max(worst, float(np.max(e / np.maximum(bd, 1e-300))))
        assert np.all(e <= bd), (label, b)
    print(f"  {label}: max err / bound over all blocks = {worst:.3f}")


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_kernel_matches_the_model(name, N, dev):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    gs = 1.0 / N
    w = M.EQ_WEIGHTS[name]
    for loss, delta in M.LOSSES:
        td = _desc(name, d, loss, delta)
        m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, w, loss, delta, gs)
        o = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5)
        bad = m["unsafe"].any(0)
        ok = ~bad
        print(f"{name} N={N} {loss}: skipped {int(bad.sum())}")
        assert bad.sum() <= 0.01 * N
        e_r = np.abs(o["r"] - m["r"])
        print(f"  r: max err / bound = {float(np.max(e_r / np.maximum(m['r_bound'], 1e-300))):.3f}")
        assert not np.any(np.isnan(o["r"])) and np.all(e_r <= m["r_bound"])
        _check_cot(o, m, ok, "cot")
        e_l = abs(float(o["loss"][0]) - (0.25 + m["loss_sum"]))
        print(f"  loss sum: err / abs sum = {e_l / max(m['loss_abs'], 1e-300):.2e}")
        assert e_l <= SUM_TOL * (0.25 + m["loss_abs"])
        e_q = np.abs(o["eq"].astype(np.float64) - (0.125 + m["eq_loss"]))
        assert np.all(e_q <= SUM_TOL * (0.125 + m["eq_abs"]))
        # a point on the wrong side of a kink changes its rbar by at most 2 |grad_scale omega| l'-range: zero when none is skipped
        slack = 2.0 * abs(gs) * max(w) * max(delta, 1.0) * np.abs(m["coef_prod"][:, bad]).sum(1)
        e_g = np.abs(o["coef"].astype(np.float64) - (-0.5 + m["coef_sums"]))
        print(f"  coef sums: max err / abs sum = {float(np.max(e_g / np.maximum(m['coef_abs'], 1e-300))):.2e}")
        assert np.all(e_g <= SUM_TOL * (0.5 + m["coef_abs"]) + slack)
        o2 = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5)  # bit-identical across calls
        for k in o:
            assert _same_bits(o[k], o2[k]), f"{k} differs between two calls"


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_cotangent_form(name, N, dev):
    """A given (E, N) cotangent replaces grad_scale omega_e l'(r_e): the loss kind, the weights and grad_scale no longer reach
    the cotangents or the coefficient sums."""
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    td = _desc(name, d, "mae", 1.0)
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, M.EQ_WEIGHTS[name], "mae", 1.0, 123.0, residual_cotangent=rbar)
    o = _run(td, d, N, dev, 123.0, rbar=d["rbar"], want=("cot", "coef"))
    _check_cot(o, m, np.ones(N, dtype=bool), "cot (given rbar)")
    assert np.all(np.abs(o["coef"] - m["coef_sums"]) <= SUM_TOL * m["coef_abs"])
    # through the engine wrapper ((N, E) cotangent), cotangents only: one launch, the same bits
    _, cot2 = E.term_residual_system_mixed(td, d["jets"], d["x"], d["t"], residual_cotangent=d["rbar"].t(), want_residual=False,
                                     want_cotangents=True)
    assert _same_bits([None if c is None else c.cpu().numpy() for c in cot2], o["cot"])


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_only_and_sums_only_forms(name, N, dev):
    """No sums, no cotangents: one launch that needs no scratch, the same residuals bit for bit; and each sum on its own,
    without the cotangent table: the same bits as in the full call."""
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, d = _case(name, N, dev)
    gs = 1.0 / N
    td = _desc(name, d)
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, M.EQ_WEIGHTS[name])
    o = _run(td, d, N, dev, 0.0, want=("r",))
    assert np.all(np.abs(o["r"] - m["r"]) <= m["r_bound"])
    full = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5)
    assert _same_bits(o["r"], full["r"])
    r, cot = E.term_residual_system_mixed(td, d["jets"], d["x"], d["t"])
    assert cot is None and r.shape == (N, n_eq) and _same_bits(np.ascontiguousarray(r.cpu().numpy().T), o["r"])
    o = _run(td, d, N, dev, gs, want=("coef",), coef0=-0.5)
    assert _same_bits(o["coef"], full["coef"])
    o = _run(td, d, N, dev, gs, want=("loss",), loss0=0.25)
    assert _same_bits(o["loss"], full["loss"])
    o = _run(td, d, N, dev, gs, want=("eq",), eq0=0.125)
    assert _same_bits(o["eq"], full["eq"])
    o = _run(td, d, N, dev, gs, want=("cot",))
    assert _same_bits(o["cot"], full["cot"])


def test_one_pair_null_blocks_and_the_unnamed_field(dev):
    """`one_pair`: only the P block (field 1, pair xz) exists; rows 0 and 1 of it are zero, row 2 is not; field 2, which no term
    names, gets all-zero blocks."""
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, d = _case("one_pair", 257, dev)
    o = _run(_desc("one_pair", d), d, 257, dev, 1.0, want=("cot",))
    C = 3
    present = [b for b in range(3 * C, 6 * C) if o["cot"][b] is not None]
    assert present == [3 * C + 3 * 1 + 1]
    P = o["cot"][present[0]]
    assert P.shape == (3, 257) and not np.any(P[:2]) and np.any(P[2])
    for b in (6, 7):  # field 2: its axis-0 block and its axis-1 block
        assert o["cot"][b] is not None and o["cot"][b].shape[1] == 257 and not np.any(o["cot"][b])
    assert o["cot"][8] is None


@pytest.mark.parametrize("N", M.SIZES)
def test_no_mixed_is_the_system_kernel_bit_for_bit(N, dev):
    """With every pair order 0 the pure-term rounding order is `pinn_term_residual_system`'s: residuals and cotangent blocks carry
    the same bits on the same inputs (the sums are held to the model's bar only)."""
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, d = _case("no_mixed", N, dev)
    C = len(nt)
    assert all(j is None for j in d["jets"][3 * C:])
    factors, eq_of = M.engine_terms(terms)
    plain = dict(d, jets=d["jets"][: 3 * C])
    entry = _lib.load().pinn_term_residual_system
    for loss, delta in M.LOSSES:
        td = _desc("no_mixed", d, loss, delta)
        ts = E.SystemTermDesc(factors, eq_of, d["coef"], dim, C, n_eq, nt, nx, M.EQ_WEIGHTS["no_mixed"], loss, delta)
        o = _run(td, d, N, dev, 1.0 / N)
        s = _run(ts, plain, N, dev, 1.0 / N, entry=entry)
        assert _same_bits(o["r"], s["r"]), loss
        assert _same_bits(o["cot"][: 3 * C], s["cot"]) and all(c is None for c in o["cot"][3 * C:]), loss
        o = _run(td, d, N, dev, 123.0, rbar=d["rbar"], want=("cot",))
        s = _run(ts, plain, N, dev, 123.0, rbar=d["rbar"], want=("cot",), entry=entry)
        assert _same_bits(o["cot"][: 3 * C], s["cot"]), loss


def test_coefficients_are_read_at_launch_time(dev):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, d = _case("elasticity2d", 257, dev)
    d2 = dict(d, coef=d["coef"].clone())
    td = _desc("elasticity2d", d2)
    r0, _ = E.term_residual_system_mixed(td, d["jets"], d["x"], d["t"])
    r0 = r0.clone()
    d2["coef"][4] = -0.5  # the coefficient of v_xy in the u-equation
    r1, _ = E.term_residual_system_mixed(td, d["jets"], d["x"], d["t"])
    c2 = coef.copy()
    c2[4] = -0.5
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, c2, jets, x, t)
    assert np.all(np.abs(r1.cpu().numpy().T - m["r"]) <= m["r_bound"])
    assert not torch.equal(r0, r1)
