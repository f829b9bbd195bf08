"""`pinn_term_residual_system_inv` against its fp64 model (tests/term_system_inv_model.py) on synthetic standard-normal blocks:
(a) `exp1`, one field, one EXP, the coefficient of the EXP term and shift and scale of the EXP learnable; (b) `euler1d`, C = E = 3,
one parameter behind two coefficients, the RECIP shift and the POW exponent learnable; (c) `caps8`, C = E = 4, dimension 3, 32
terms, 8 parameters: one shared by three terms and a nonlinear scale, a learnable entry on a function outside the mask (whose
numbers are NaN on the device), the chain nl1(nl0(.)) with both shifts learnable — x the sizes 1, 255, 256, 257 and 64 x 256 + 3
x the three loss kinds, with and without `residual_cotangent`, `jet_cotangents`, `coef_grads`, `eq_loss_sums`.

Per point, the residual of every equation and every cotangent row are within the model's bound; the loss sums and the
coefficient sums are within the sibling's 1e-6 of the sum of the absolute summands; `param_grads` is within 1e-6 of the sum of
its absolute summands plus the model's propagated per-point bounds (plus, under mae / Huber, what the points within their bound
of a kink can move it by: zero when none is unsafe), and accumulates onto a non-zero start value.  Outputs are poisoned with
NaN and carry guard floats that must stay NaN; two calls are bit-identical; the sums have the same bits with `jet_cotangents`
NULL; with n_params = 0 every output is bit-identical to `pinn_term_residual_system_nl`; `param_values` rewritten in place
between two calls is followed.  Every test prints its largest error / bound ratio."""

import ctypes

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import term_system_inv_model as M
import term_system_nl_model as NM
from pinnrl_amd import _lib
from pinnrl_amd import engine as E

pytestmark = pytest.mark.gpu

SUM_TOL = M.SUM_TOL
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
        a = M.inputs(name, N)
        dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, pv, cp, npar = a
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar), ("fn", fn), ("nlp", params),
                                                         ("pv", pv))}
        d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
        _cache[key] = a + (d,)
    return _cache[key]


def _no_fn(x, t):
    raise AssertionError("the kernel tests pass the function values themselves")


def _desc(name, d, loss="mse", delta=1.0):
    dim, nt, nx, pair, n_eq, terms, _, K, nl, pv, cp, npar = M.PROGRAMS[name]
    factors, eq_of = M.engine_terms(terms)
    rows = M.engine_nonlinear([r[:2] for r in nl], [r[2:] for r in nl])
    return E.InvSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, rows, M.EQ_WEIGHTS[name],
                               loss, delta, nl_values=d["nlp"], param_values=d["pv"], coef_param=cp, nl_param=npar)


def _poisoned(n, dev):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def _run(td, d, N, dev, grad_scale, rbar=None, want=("r", "loss", "eq", "cot", "coef", "pg"), loss0=0.0, eq0=0.0, coef0=0.0, pg0=0.0,
         sibling=False):
    """One raw call through the C ABI with poisoned, guarded outputs.  Returns host arrays (cot: a list of blocks).  sibling:
    `pinn_term_residual_system_nl` (td an `NlSystemTermDesc`) instead."""
    lib = _lib.load()
    T, Eq = td.desc.n_terms, td.n_equations
    P = 0 if sibling else int(td.desc.n_params)
    rows = [None if j is None else j.shape[0] for j in d["jets"]]
    nb = len(rows)
    r = _poisoned(Eq * N, dev) if "r" in want else None
    cot = [None if k is None else _poisoned(k * N, dev) for k in rows] if "cot" in want else None
    loss = _poisoned(1, dev) if "loss" in want else None
    eq = _poisoned(Eq, dev) if "eq" in want else None
    cg = _poisoned(_lib.PINN_SYSTEM_MAX_TERMS, dev) if "coef" in want else None
    pg = _poisoned(_lib.PINN_SYSTEM_MAX_PARAMS, dev) if ("pg" in want and not sibling and P) else None
    if loss is not None:
        loss[0] = loss0
    if eq is not None:
        eq[:Eq] = eq0
    if cg is not None:
        cg[:T] = coef0
    if pg is not None:
        pg[:P] = pg0
    doubles = _lib.PINN_SYSTEM_SCRATCH_DOUBLES if sibling else _lib.PINN_SYSTEM_INV_SCRATCH_DOUBLES
    scratch = torch.full((doubles + GUARD,), float("nan"), dtype=torch.float64, device=dev)
    opt = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
    jptr = (ctypes.c_void_p * nb)(*[opt(j) for j in d["jets"]])
    cptr = (ctypes.c_void_p * nb)(*[opt(c) for c in cot]) if cot is not None else None
    sums = any(v is not None for v in (loss, eq, cg, pg))
    head = (ctypes.byref(td.desc), d["coef"].data_ptr(), jptr, d["x"].data_ptr(), d["t"].data_ptr(),
            opt(d.get("fn")) if td.functions else None, opt(d.get("nlp")))
    sp = scratch.data_ptr() if sums else None
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if sibling:
            rc = lib.pinn_term_residual_system_nl(*head, N, float(grad_scale), opt(rbar), opt(r), opt(loss), opt(eq), cptr, opt(cg), sp, st)
        else:
            rc = lib.pinn_term_residual_system_inv(*head, opt(d.get("pv")) if P else None, N, float(grad_scale), opt(rbar), opt(r),
                                                   opt(loss), opt(eq), cptr, opt(cg), opt(pg), sp, st)
    _lib.check(rc)
    torch.cuda.synchronize(dev)
    out = {}
    for k, v, n in (("r", r, Eq * N), ("loss", loss, 1), ("eq", eq, Eq), ("coef", cg, T), ("pg", pg, P)):
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
    assert np.all(np.isnan(scratch[doubles:].cpu().numpy())), "scratch: written past its doubles"
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
        assert np.all(e <= bd), (label, b, float(np.max(e / np.maximum(bd, 1e-300))))
    print(f"  {label}: max err / bound over all blocks = {worst:.3f}")


def _check_pg(o, m, start, label):
    """param_grads against the model: 1e-6 of the absolute summands, the propagated per-point bounds, the kink slack."""
    tol = SUM_TOL * (abs(start) + m["param_abs"]) + m["param_bound"] + m["param_slack"]
    e = np.abs(o["pg"].astype(np.float64) - (start + m["param_grads"]))
    print(f"  {label}: max err / tolerance = {float(np.max(e / np.maximum(tol, 1e-300))):.3f}; max err / abs sum = "
          f"{float(np.max(e / np.maximum(m['param_abs'], 1e-300))):.2e}")
    assert np.all(e <= tol), (label, e, tol)


def _model(a, name, loss="mse", delta=1.0, gs=1.0, rbar=None, pv=None):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, _, fn, nl, params, pv0, cp, npar = a[:17]
    return M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, pv0 if pv is None else pv, cp, npar,
                      M.EQ_WEIGHTS[name], loss, delta, gs, residual_cotangent=rbar)


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_kernel_matches_the_model(name, N, dev):
    a = _case(name, N, dev)
    d = a[-1]
    gs = 1.0 / N
    w = M.EQ_WEIGHTS[name]
    for loss, delta in M.LOSSES:
        td = _desc(name, d, loss, delta)
        m = _model(a, name, loss, delta, gs)
        o = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5, pg0=0.75)
        assert _all_finite(o), "an output is not finite (a function outside the mask was evaluated?)"
        bad = m["unsafe"].any(0)
        ok = ~bad
        print(f"{name} N={N} {loss}: skipped {int(bad.sum())}")
        assert bad.sum() <= 0.01 * N
        e_r = np.abs(o["r"] - m["r"])
        ratio = float(np.max(e_r / np.maximum(m["r_bound"], 1e-300)))
        print(f"  r: max err / bound = {ratio:.3f}")
        assert np.all(e_r <= m["r_bound"]), ratio
        _check_cot(o, m, ok, "cot")
        e_l = abs(float(o["loss"][0]) - (0.25 + m["loss_sum"]))
        assert e_l <= SUM_TOL * (0.25 + m["loss_abs"])
        e_q = np.abs(o["eq"].astype(np.float64) - (0.125 + m["eq_loss"]))
        assert np.all(e_q <= SUM_TOL * (0.125 + m["eq_abs"]))
        e_g = np.abs(o["coef"].astype(np.float64) - (-0.5 + m["coef_sums"]))
        print(f"  coef sums: max err / abs sum = {float(np.max(e_g / np.maximum(m['coef_abs'], 1e-300))):.2e}")
        assert np.all(e_g <= SUM_TOL * (0.5 + m["coef_abs"]) + m["G_bound"] + m["G_slack"])
        _check_pg(o, m, 0.75, "param_grads (accumulated onto 0.75)")
        o2 = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5, pg0=0.75)  # bit-identical across calls
        for k in o:
            assert _same_bits(o[k], o2[k]), f"{k} differs between two calls"


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_cotangent_form_and_output_combinations(name, N, dev):
    """A given (E, N) cotangent replaces grad_scale omega_e l'(r_e) in the cotangents, the coefficient sums and param_grads alike.
    Every output on its own, and param_grads without `jet_cotangents`, carry the bits of the full call."""
    a = _case(name, N, dev)
    d = a[-1]
    td = _desc(name, d, "mae", 1.0)
    m = _model(a, name, "mae", 1.0, 123.0, rbar=a[10])
    full = _run(td, d, N, dev, 123.0, rbar=d["rbar"])
    assert _all_finite(full)
    _check_cot(full, m, np.ones(N, dtype=bool), "cot (given rbar)")
    assert np.all(np.abs(full["coef"] - m["coef_sums"]) <= SUM_TOL * m["coef_abs"])
    _check_pg(full, m, 0.0, "param_grads (given rbar)")
    assert np.all(np.abs(full["r"] - m["r"]) <= m["r_bound"])
    for want in (("pg",), ("pg", "coef"), ("pg", "cot"), ("pg", "eq", "r"), ("coef",), ("cot",), ("loss",), ("r",)):
        o = _run(td, d, N, dev, 123.0, rbar=d["rbar"], want=want)
        for k in want:
            assert _same_bits(o[k], full[k]), (want, k)
    # the loss form: the sums alone against the full call
    gs = 1.0 / N
    for loss, delta in M.LOSSES:
        tl = _desc(name, d, loss, delta)
        f2 = _run(tl, d, N, dev, gs)
        for want in (("pg",), ("pg", "loss"), ("coef", "eq")):
            o = _run(tl, d, N, dev, gs, want=want)
            for k in want:
                assert _same_bits(o[k], f2[k]), (loss, want, k)
    # through the engine front end ((N, E) cotangent): the same bits
    pg = torch.zeros(8, dtype=torch.float32, device=dev)
    r, cot2 = E.term_residual_system_inv(td, d["jets"], d["fn"] if td.functions else None, d["nlp"], d["pv"], d["x"], d["t"],
                                         residual_cotangent=d["rbar"].t(), want_cotangents=True, param_grads=pg)
    assert _same_bits([None if c is None else c.cpu().numpy() for c in cot2], full["cot"])
    assert _same_bits(pg.cpu().numpy()[: len(full["pg"])], full["pg"]) and r.shape == (N, td.n_equations)


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(NM.PROGRAMS))
def test_no_parameters_is_the_sibling_kernel_bit_for_bit(name, N, dev):
    """The sibling's programs through the new entry point with n_params = 0 and NULL parameter pointers: residuals, every
    cotangent block and the sums carry the bits of `pinn_term_residual_system_nl`, in the loss form and in the given-cotangent
    form."""
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params = NM.inputs(name, N)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar), ("fn", fn), ("nlp", params))}
    d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
    K = NM.PROGRAMS[name][7]
    factors, eq_of = NM.engine_terms(terms)
    rows = NM.engine_nonlinear(nl, params)
    w = NM.EQ_WEIGHTS[name]
    for loss, delta in M.LOSSES:
        ts = E.NlSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, rows, w, loss, delta,
                                nl_values=d["nlp"])
        ti = E.InvSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, rows, w, loss, delta,
                                 nl_values=d["nlp"])
        keys = ("r", "loss", "eq", "cot", "coef")
        s = _run(ts, d, N, dev, 1.0 / N, want=keys, sibling=True)
        o = _run(ti, d, N, dev, 1.0 / N, want=keys)
        for k in keys:
            assert _same_bits(o[k], s[k]), (k, loss)
        s_c = _run(ts, d, N, dev, 123.0, rbar=d["rbar"], want=("cot", "coef"), sibling=True)
        o_c = _run(ti, d, N, dev, 123.0, rbar=d["rbar"], want=("cot", "coef"))
        assert _same_bits(o_c["cot"], s_c["cot"]) and _same_bits(o_c["coef"], s_c["coef"]), loss
        assert _same_bits(_run(ti, d, N, dev, 0.0, want=("r",))["r"], s["r"])


@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_param_values_are_read_at_launch_time(name, dev):
    a = _case(name, 257, dev)
    d = dict(a[-1], pv=a[-1]["pv"].clone())
    td = _desc(name, d)
    o0 = _run(td, d, 257, dev, 1.0 / 257)
    pv2 = a[14].copy()
    pv2 *= np.float32(1.03125)  # keeps every restricted argument in its domain
    d["pv"].copy_(torch.from_numpy(pv2))  # in place: the descriptor and the call keep the tensor
    o1 = _run(td, d, 257, dev, 1.0 / 257)
    m = _model(a, name, gs=1.0 / 257, pv=pv2)
    assert np.all(np.abs(o1["r"] - m["r"]) <= m["r_bound"]) and not _same_bits(o0["r"], o1["r"])
    _check_cot(o1, m, np.ones(257, dtype=bool), "cot (rewritten parameters)")
    _check_pg(o1, m, 0.0, "param_grads (rewritten parameters)")
    assert not _same_bits(o0["pg"], o1["pg"])
