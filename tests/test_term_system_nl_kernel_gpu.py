"""`pinn_term_residual_system_nl` against its fp64 model (tests/term_system_nl_model.py) on synthetic standard-normal blocks and
function rows with O(1) coefficients: (a) `bratu1d`, C = 1, one EXP; (b) `euler1d`, C = E = 3, RECIP of rho in two terms and a
POW; (c) `caps`, C = E = 4, dimension 3, 32 terms, all four known functions and all four nonlinear slots as one chain
nl3(nl2(nl1(nl0(u_xy)))), one nonlinear factor twice in a term, a term nonlinear x function x trig x coordinate — and
`caps_tree`, the same terms over nl3(nl0(u_x)) and nl2(nl1(u_xy)), since a chain of four has one field source only; every
operation appears in (a) .. (c); (d) `masked`, four declared, only nl2 named, its source nl1, nl0 and nl3 LOG with NaN
parameters; (e) the sibling's programs with n_nonlinear 0 and 4 and none named — x the sizes 1, 255, 256, 257 and
64 x 256 + 3 x the three loss kinds, with and without `residual_cotangent`, `coef_grads` and `eq_loss_sums`.

Per point, the residual of every equation and every cotangent row of all 6 C blocks are within the model's bound (whose U_g are
the OpenCL 1.2 limits, not measured here); the rows the model marks untouched are exactly zero; the weighted loss sum, the
per-equation sums and the coefficient sums are within the sibling's 1e-6 of the sum of the absolute summands.  Outputs are
poisoned with NaN and carry guard floats that must stay NaN; two calls are bit-identical.  On (d) every output is finite.  On
(e) residuals, cotangent blocks and sums are bit-identical to `pinn_term_residual_system_fn` on the same inputs.  Coefficients
and parameters are read at launch time.  For mae and Huber, points whose fp64 |r_e| lies within its bound of 0 / delta may take
the other branch of l' on the device: they are skipped (tests/test_term_system_nl_cpu.py shows on the model alone that the seeds
leave at most 1 %).  Every test prints its largest error / bound ratio."""

import ctypes

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import term_system_fn_model as FM
import term_system_nl_model as M
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
        dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params = M.inputs(name, N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar), ("fn", fn), ("nlp", params))}
        d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
        _cache[key] = (dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, d)
    return _cache[key]


def _no_fn(x, t):
    raise AssertionError("the kernel tests pass the function values themselves")


def _desc(name, d, loss="mse", delta=1.0):
    dim, nt, nx, pair, n_eq, terms, _, K, nl = M.PROGRAMS[name]
    factors, eq_of = M.engine_terms(terms)
    rows = M.engine_nonlinear([r[:2] for r in nl], [r[2:] for r in nl])
    return E.NlSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, rows, M.EQ_WEIGHTS[name],
                              loss, delta, nl_values=d["nlp"])


def _poisoned(n, dev):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def _run(td, d, N, dev, grad_scale, rbar=None, want=("r", "loss", "eq", "cot", "coef"), loss0=0.0, eq0=0.0, coef0=0.0, sibling=False):
    """One raw call through the C ABI with poisoned, guarded outputs.  Returns host arrays (cot: a list of blocks).  sibling:
    `pinn_term_residual_system_fn` (td a `FnSystemTermDesc`) instead."""
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
    head = (ctypes.byref(td.desc), d["coef"].data_ptr(), jptr, d["x"].data_ptr(), d["t"].data_ptr(), opt(d.get("fn")))
    tail = (N, float(grad_scale), opt(rbar), opt(r), opt(loss), opt(eq), cptr, opt(cg), scratch.data_ptr() if sums else None,
            torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if sibling:
            rc = lib.pinn_term_residual_system_fn(*head, *tail)
        else:
            rc = lib.pinn_term_residual_system_nl(*head, opt(d.get("nlp")), *tail)
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
        assert np.all(e <= bd), (label, b, float(np.max(e / np.maximum(bd, 1e-300))))
    print(f"  {label}: max err / bound over all blocks = {worst:.3f}")


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_kernel_matches_the_model(name, N, dev):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, d = _case(name, N, dev)
    gs = 1.0 / N
    w = M.EQ_WEIGHTS[name]
    for loss, delta in M.LOSSES:
        td = _desc(name, d, loss, delta)
        m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, w, loss, delta, gs)
        o = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5)
        assert _all_finite(o), "an output is not finite (a function outside the mask was evaluated, or an unnamed row read?)"
        bad = m["unsafe"].any(0)
        ok = ~bad
        print(f"{name} N={N} {loss}: skipped {int(bad.sum())}")
        assert bad.sum() <= 0.01 * N
        e_r = np.abs(o["r"] - m["r"])
        ratio = float(np.max(e_r / np.maximum(m["r_bound"], 1e-300)))
        print(f"  r: max err / bound = {ratio:.3f}")
        assert not np.any(np.isnan(o["r"])) and np.all(e_r <= m["r_bound"]), ratio
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
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, d = _case(name, N, dev)
    td = _desc(name, d, "mae", 1.0)
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, M.EQ_WEIGHTS[name], "mae", 1.0, 123.0,
                   residual_cotangent=rbar)
    o = _run(td, d, N, dev, 123.0, rbar=d["rbar"], want=("cot", "coef"))
    assert _all_finite(o)
    _check_cot(o, m, np.ones(N, dtype=bool), "cot (given rbar)")
    assert np.all(np.abs(o["coef"] - m["coef_sums"]) <= SUM_TOL * m["coef_abs"])
    # through the engine front end ((N, E) cotangent), cotangents only: one launch, the same bits
    _, cot2 = E.term_residual_system_nl(td, d["jets"], d["fn"] if td.functions else None, d["nlp"], d["x"], d["t"],
                                        residual_cotangent=d["rbar"].t(), want_residual=False, want_cotangents=True)
    assert _same_bits([None if c is None else c.cpu().numpy() for c in cot2], o["cot"])


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_residual_only_and_sums_only_forms(name, N, dev):
    """No sums, no cotangents: one launch that needs no scratch, the same residuals bit for bit; and each sum on its own,
    without the cotangent table: the same bits as in the full call."""
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, d = _case(name, N, dev)
    gs = 1.0 / N
    td = _desc(name, d)
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, M.EQ_WEIGHTS[name])
    o = _run(td, d, N, dev, 0.0, want=("r",))
    assert np.all(np.abs(o["r"] - m["r"]) <= m["r_bound"])
    full = _run(td, d, N, dev, gs, loss0=0.25, eq0=0.125, coef0=-0.5)
    assert _same_bits(o["r"], full["r"])
    r, cot = E.term_residual_system_nl(td, d["jets"], d["fn"] if td.functions else None, d["nlp"], d["x"], d["t"])
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
        dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn = FM.inputs(name, N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("coef", coef), ("x", x), ("t", t), ("rbar", rbar), ("fn", fn))}
        d["jets"] = [None if j is None else torch.from_numpy(j).to(dev) for j in jets]
        _sib[key] = (dim, nt, nx, pair, n_eq, terms, d)
    return _sib[key]


@pytest.mark.parametrize("N", M.SIZES)
@pytest.mark.parametrize("name", sorted(FM.PROGRAMS))
def test_no_nonlinear_factor_named_is_the_sibling_kernel_bit_for_bit(name, N, dev):
    """(e) The sibling's programs through the new entry point, with n_nonlinear 0 (nl_params NULL) and 4 (four LOG declarations
    with NaN parameters that no term names): residuals, every cotangent block and the sums carry the bits of
    `pinn_term_residual_system_fn` on the same inputs, in the loss form and in the given-cotangent form."""
    dim, nt, nx, pair, n_eq, terms, d = _sibling_case(name, N, dev)
    K = FM.PROGRAMS[name][7]
    factors, eq_of = FM.engine_terms(terms)
    w = FM.EQ_WEIGHTS[name]
    nan_params = torch.full((4, 3), float("nan"), dtype=torch.float32, device=dev)
    four = [("log", (0, "u"), 0.0, 1.0, 1.0), ("log", "nl0", 0.0, 1.0, 1.0), ("log", (0, "u"), 0.0, 1.0, 1.0), ("log", "nl2", 0.0, 1.0, 1.0)]
    for loss, delta in M.LOSSES:
        ts = E.FnSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, w, loss, delta)
        s = _run(ts, d, N, dev, 1.0 / N, sibling=True)
        s_c = _run(ts, d, N, dev, 123.0, rbar=d["rbar"], want=("cot",), sibling=True)
        for nl, nlp in (((), None), (four, nan_params)):
            td = E.NlSystemTermDesc(factors, eq_of, d["coef"], dim, len(nt), n_eq, nt, nx, pair, [_no_fn] * K, nl, w, loss, delta,
                                    nl_values=nlp)
            o = _run(td, dict(d, nlp=nlp), N, dev, 1.0 / N)
            for k in ("r", "cot", "loss", "eq", "coef"):
                assert _same_bits(o[k], s[k]), (k, loss, len(nl))
            o = _run(td, dict(d, nlp=nlp), N, dev, 123.0, rbar=d["rbar"], want=("cot",))
            assert _same_bits(o["cot"], s_c["cot"]), (loss, len(nl))


def test_coefficients_and_parameters_are_read_at_launch_time(dev):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, d = _case("euler1d", 257, dev)
    d2 = dict(d, coef=d["coef"].clone(), nlp=d["nlp"].clone())
    td = _desc("euler1d", d2)
    r0, _ = E.term_residual_system_nl(td, d["jets"], None, d2["nlp"], d["x"], d["t"])
    r0 = r0.clone()
    d2["coef"][5] = -0.5      # the coefficient of p_x / rho
    d2["nlp"][0, 0] = 3.5     # the shift of 1 / rho
    d2["nlp"][1, 2] = 1.6667  # the exponent of the POW
    r1, _ = E.term_residual_system_nl(td, d["jets"], None, d2["nlp"], d["x"], d["t"])
    c2, p2 = coef.copy(), params.copy()
    c2[5] = -0.5
    p2[0, 0] = 3.5
    p2[1, 2] = 1.6667
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, c2, jets, x, t, None, nl, p2)
    assert np.all(np.abs(r1.cpu().numpy().T - m["r"]) <= m["r_bound"])
    assert not torch.equal(r0, r1)


def test_front_end_refusals(dev):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, d = _case("euler1d", 255, dev)
    td = _desc("euler1d", d)
    call = lambda **kw: E.term_residual_system_nl(td, kw.get("jets", d["jets"]), kw.get("fn"), kw.get("nlp", d["nlp"]),  # noqa: E731
                                                  kw.get("x", d["x"]), d["t"], residual_cotangent=kw.get("rbar"))
    with pytest.raises(ValueError, match="nl_params is None but the descriptor has 2 nonlinear functions"):
        call(nlp=None)
    for bad in (d["nlp"][:1], d["nlp"].double(), d["nlp"].t().contiguous().t(), d["nlp"].reshape(-1)):
        with pytest.raises(ValueError, match=r"nl_params must be a contiguous float32 \(2, 3\) tensor"):
            call(nlp=bad)
    with pytest.raises(RuntimeError, match="ROCm device|same device"):
        call(nlp=d["nlp"].cpu())
    with pytest.raises(ValueError, match=r"fn_values must be a contiguous float32 \(0, N\) tensor"):
        call(fn=torch.zeros((1, 255), device=dev))
    with pytest.raises(ValueError, match=r"block 0 \(field 0, axis 0\) must be a contiguous float32 \(3, 255\) tensor"):
        call(jets=[d["jets"][0].double()] + d["jets"][1:])
    with pytest.raises(ValueError, match=r"x is \(N, 1\) and t holds N values"):
        call(x=d["x"][:100])
    with pytest.raises(ValueError, match=r"residual_cotangent is \(N, E\) = \(255, 3\)"):
        call(rbar=d["rbar"])  # (E, N) where (N, E) is expected
    # a descriptor without nonlinear functions takes nl_params None
    dim, nt, nx, pair, n_eq, terms, d2 = _sibling_case("source1d", 255, dev)
    factors, eq_of = FM.engine_terms(terms)
    t0 = E.NlSystemTermDesc(factors, eq_of, d2["coef"], dim, 1, n_eq, nt, nx, pair, [_no_fn] * 2)
    r, _ = E.term_residual_system_nl(t0, d2["jets"], d2["fn"], None, d2["x"], d2["t"])
    assert r.shape == (255, 1) and bool(torch.isfinite(r).all())
