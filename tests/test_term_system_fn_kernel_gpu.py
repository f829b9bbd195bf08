"""`pinn_term_residual_system_fn` against its fp64 model (tests/term_system_fn_model.py) on synthetic standard-normal blocks and
function rows with O(1) coefficients: (a) `source1d`, C = 1 in 1-D, a source-only term and g u_xx; (b) `elasticity_force`,
C = E = 2, 2-D elasticity with a body force per equation and a variable modulus multiplying a mixed factor; (c) `caps`, C = E = 4,
dimension 3, 32 terms, all four functions, one function twice in a term, function x trig x coordinate; (d) `one_named`,
n_functions = 4 with only function 2 named and the other rows NaN; (e) the sibling's programs with n_functions 0 and 4 and no
function named — x the sizes 1, 255, 256, 257 and 64 x 256 + 3 x the three loss kinds, with and without `residual_cotangent`,
`coef_grads` and `eq_loss_sums`.

Per point, the residual of every equation and every cotangent row of all 6 C blocks are within the model's bound; the rows the
model marks untouched are exactly zero; the weighted loss sum, the per-equation sums and the coefficient sums are within the
sibling's 1e-6 of the sum of the absolute summands.  Outputs are poisoned with NaN and carry guard floats that must stay NaN;
two calls are bit-identical.  On (d) every output is finite.  On (e) residuals and cotangent blocks are bit-identical to
`pinn_term_residual_system_mixed` on the same inputs.  Coefficients and function values are read at launch time.  For mae and
Huber, points whose fp64 |r_e| lies within its bound of 0 / delta may take the other branch of l' on the device: they are
skipped (tests/test_term_system_fn_cpu.py shows on the model alone that the seeds leave at most 1 %)."""

import ctypes

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import term_system_fn_model as M
import term_system_mixed_model as MM
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
        dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn = M.inputs(name, N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar), ("fn", fn))}
        d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
        _cache[key] = (dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, d)
    return _cache[key]


def _no_fn(x, t):
    raise AssertionError("the kernel tests pass the function values themselves")


def _desc(name, d, loss="mse", delta=1.0):
    dim, nt, nx, pair, n_eq, terms, _, K = M.PROGRAMS[name]
    factors, eq_of = M.engine_terms(terms)
    return E.FnSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, M.EQ_WEIGHTS[name], loss, delta)


def _poisoned(n, dev):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def _run(td, d, N, dev, grad_scale, rbar=None, want=("r", "loss", "eq", "cot", "coef"), loss0=0.0, eq0=0.0, coef0=0.0, sibling=False):
    """One raw call through the C ABI with poisoned, guarded outputs.  Returns host arrays (cot: a list of blocks).  sibling:
    `pinn_term_residual_system_mixed` (td a `MixedSystemTermDesc`) instead."""
    lib = _lib.load()
    T, Eq = td.desc.n_terms, td.n_equations
    rows = [None if j is None else j.shape[0] for j in d["jets"]]
    nb = len(rows)
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
    head = (ctypes.byref(td.desc), d["coef"].data_ptr(), jptr, d["x"].data_ptr(), d["t"].data_ptr())
    tail = (N, float(grad_scale), opt(rbar), opt(r), opt(loss), opt(eq), cptr, opt(cg), scratch.data_ptr() if sums else None,
            torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if sibling:
            rc = lib.pinn_term_residual_system_mixed(*head, *tail)
        else:
            rc = lib.pinn_term_residual_system_fn(*head, opt(d.get("fn")), *tail)
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


def _all_finite(o):
    return all(np.all(np.isfinite(c)) for v in o.values() for c in (v if isinstance(v, list) else [v]) if c is not None)


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
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, d = _case(name, N, dev)
    gs = 1.0 / N
    w = M.EQ_WEIGHTS[name]
    for loss, delta in M.LOSSES:
        td = _desc(name, d, loss, delta)
        m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, w, loss, delta, gs)
        o = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5)
        assert _all_finite(o), "an output is not finite (a function row that no term names was read?)"
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
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, d = _case(name, N, dev)
    td = _desc(name, d, "mae", 1.0)
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, M.EQ_WEIGHTS[name], "mae", 1.0, 123.0, residual_cotangent=rbar)
    o = _run(td, d, N, dev, 123.0, rbar=d["rbar"], want=("cot", "coef"))
    assert _all_finite(o)
    _check_cot(o, m, np.ones(N, dtype=bool), "cot (given rbar)")
    assert np.all(np.abs(o["coef"] - m["coef_sums"]) <= SUM_TOL * m["coef_abs"])
    # through the engine front end ((N, E) cotangent), cotangents only: one launch, the same bits
    _, cot2 = E.term_residual_system_fn(td, d["jets"], d["fn"], d["x"], d["t"], residual_cotangent=d["rbar"].t(), want_residual=False,
                                        want_cotangents=True)
    assert _same_bits([None if c is None else c.cpu().numpy() for c in cot2], o["cot"])


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_only_and_sums_only_forms(name, N, dev):
    """No sums, no cotangents: one launch that needs no scratch, the same residuals bit for bit; and each sum on its own,
    without the cotangent table: the same bits as in the full call."""
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, d = _case(name, N, dev)
    gs = 1.0 / N
    td = _desc(name, d)
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, M.EQ_WEIGHTS[name])
    o = _run(td, d, N, dev, 0.0, want=("r",))
    assert np.all(np.abs(o["r"] - m["r"]) <= m["r_bound"])
    full = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5)
    assert _same_bits(o["r"], full["r"])
    r, cot = E.term_residual_system_fn(td, d["jets"], d["fn"], d["x"], d["t"])
    assert cot is None and r.shape == (N, n_eq) and _same_bits(np.ascontiguousarray(r.cpu().numpy().T), o["r"])
    o = _run(td, d, N, dev, gs, want=("coef",), coef0=-0.5)
    assert _same_bits(o["coef"], full["coef"])
    o = _run(td, d, N, dev, gs, want=("loss",), loss0=0.25)
    assert _same_bits(o["loss"], full["loss"])
    o = _run(td, d, N, dev, gs, want=("eq",), eq0=0.125)
    assert _same_bits(o["eq"], full["eq"])
    o = _run(td, d, N, dev, gs, want=("cot",))
    assert _same_bits(o["cot"], full["cot"])


_sib = {}


def _sibling_case(name, N, dev):
    key = (name, N)
    if key not in _sib:
        dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar = MM.inputs(name, N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar))}
        d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
        _sib[key] = (dim, nt, nx, pair, n_eq, terms, d)
    return _sib[key]


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(MM.PROGRAMS))
def test_no_function_named_is_the_sibling_kernel_bit_for_bit(name, N, dev):
    """(e) The sibling's programs through the new entry point, with n_functions 0 (fn_values NULL) and 4 (four rows of NaN that no
    term names): residuals and every cotangent block carry the bits of `pinn_term_residual_system_mixed` on the same inputs, in
    the loss form and in the given-cotangent form; the sums are the same bits too (the same partials in the same order)."""
    dim, nt, nx, pair, n_eq, terms, d = _sibling_case(name, N, dev)
    factors, eq_of = MM.engine_terms(terms)
    w = MM.EQ_WEIGHTS[name]
    nan_rows = torch.full((4, N), float("nan"), dtype=torch.float32, device=dev)
    for loss, delta in M.LOSSES:
        ts = E.MixedSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, w, loss, delta)
        s = _run(ts, d, N, dev, 1.0 / N, sibling=True)
        s_c = _run(ts, d, N, dev, 123.0, rbar=d["rbar"], want=("cot",), sibling=True)
        for K, fn in ((0, None), (4, nan_rows)):
            td = E.FnSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, w, loss, delta)
            o = _run(td, dict(d, fn=fn), N, dev, 1.0 / N)
            for k in ("r", "cot", "loss", "eq", "coef"):
                assert _same_bits(o[k], s[k]), (k, loss, K)
            o = _run(td, dict(d, fn=fn), N, dev, 123.0, rbar=d["rbar"], want=("cot",))
            assert _same_bits(o["cot"], s_c["cot"]), (loss, K)


def test_coefficients_and_function_values_are_read_at_launch_time(dev):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, d = _case("elasticity_force", 257, dev)
    d2 = dict(d, coef=d["coef"].clone(), fn=d["fn"].clone())
    td = _desc("elasticity_force", d2)
    r0, _ = E.term_residual_system_fn(td, d["jets"], d2["fn"], d["x"], d["t"])
    r0 = r0.clone()
    d2["coef"][4] = -0.5   # the coefficient of a v_xy in the u-equation
    d2["fn"][2].mul_(2.0)  # the modulus a
    d2["fn"][0].fill_(0.75)  # the body force of the u-equation
    r1, _ = E.term_residual_system_fn(td, d["jets"], d2["fn"], d["x"], d["t"])
    c2, f2 = coef.copy(), fn.copy()
    c2[4] = -0.5
    f2[2] *= 2.0
    f2[0] = 0.75
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, c2, jets, x, t, f2)
    assert np.all(np.abs(r1.cpu().numpy().T - m["r"]) <= m["r_bound"])
    assert not torch.equal(r0, r1)


def test_front_end_refusals(dev):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, d = _case("source1d", 255, dev)
    td = _desc("source1d", d)
    call = lambda **kw: E.term_residual_system_fn(td, kw.get("jets", d["jets"]), kw.get("fn", d["fn"]), kw.get("x", d["x"]), d["t"],  # noqa: E731
                                                  residual_cotangent=kw.get("rbar"))
    with pytest.raises(ValueError, match="fn_values is None but the descriptor has 2 functions"):
        call(fn=None)
    for bad in (d["fn"][:1], d["fn"].double(), d["fn"].t().contiguous().t(), d["fn"].reshape(-1)):
        with pytest.raises(ValueError, match=r"fn_values must be a contiguous float32 \(2, N\) tensor"):
            call(fn=bad)
    with pytest.raises(ValueError, match="fn_values holds 254 values per function, the jets 255"):
        call(fn=d["fn"][:, :254].contiguous())
    with pytest.raises(RuntimeError, match="ROCm device|same device"):
        call(fn=d["fn"].cpu())
    with pytest.raises(ValueError, match=r"block 0 \(field 0, axis 0\) must be a contiguous float32 \(4, 255\) tensor"):
        call(jets=[d["jets"][0].double()] + d["jets"][1:])
    with pytest.raises(ValueError, match=r"block 0 \(field 0, axis 0\) must be"):
        call(jets=[d["jets"][0].t().contiguous().t()] + d["jets"][1:])
    with pytest.raises(ValueError, match=r"x is \(N, 1\) and t holds N values"):
        call(x=d["x"][:100])
    with pytest.raises(ValueError, match=r"residual_cotangent is \(N, E\) = \(255, 1\)"):
        call(rbar=d["rbar"])  # (E, N) where (N, E) is expected... for E = 1 the shapes differ as (1, 255) and (255, 1)
    # a descriptor without functions takes fn_values None
    factors, eq_of = MM.engine_terms(MM.PROGRAMS["elasticity2d"][5])
    dim, nt, nx, pair, n_eq, terms, d2 = _sibling_case("elasticity2d", 255, dev)
    t0 = E.FnSystemTermDesc(factors, eq_of, d2["coef"], dim, 2, n_eq, nt, nx, pair)
    r, _ = E.term_residual_system_fn(t0, d2["jets"], None, d2["x"], d2["t"])
    assert r.shape == (255, 2) and bool(torch.isfinite(r).all())
