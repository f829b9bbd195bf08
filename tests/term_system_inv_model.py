"""fp64 specification of `pinn_term_residual_system_inv` (include/pinn_jet.h) in numpy, with per-point error bounds.

A program is a program of tests/term_system_nl_model.py plus the parameters: `param_values` (P,), `coef_param` (per term -1 or a
parameter index) and `nl_param` (per nonlinear function three such entries: shift, scale, exponent).  The stored coefficient
and the stored entries of a triple are SCALES where the index is >= 0: the effective number is scale * parameter, ONE float32
rounding (`effective`), and an IEEE product has one result, so the model forms the very float32 number the device forms and hands
it to `term_system_nl_model.evaluate`: residuals, losses, cotangent blocks, `coef_sums` (G) and their bounds are that model's, on
the effective values.  What is new here:

    wbar_k      the complete cotangent of w_k (the term summands, then the pushes of the later functions in descending k), with the
                bound the sibling gives every accumulator: count EPS Bw + Bd + Rw (1 + count EPS);
    H_k0 = sum_n wbar_k g_k'(arg_k),   H_k1 = sum_n (wbar_k g_k'(arg_k)) s_k,   H_k2 = sum_n (wbar_k w_k) log(arg_k)   (pow only)
    param_grads[p] = sum_{m: coef_param[m] = p} coef[m] G_m + sum_{(k, j): nl_param[k][j] = p} nl_params[k][j] H_kj.

Per-point bounds of the H summands are first order, from the pieces the sibling model already bounds: err(wbar), err(slope) =
err(d_k) / |scale| (`U_G` of the slope's library function inside), err(s_k), err(w_k), and for log(arg) U_G["log"] EPS |log| +
err(arg) / |arg|; every product adds one EPS.  A sum is compared to 1e-6 of the sum of its absolute summands (the sibling's
SUM_TOL) plus the sum of these bounds; under mae / Huber, a point within its bound of a kink of l' may carry another rbar on the
device, by at most 2 |grad_scale| omega_e max(delta, 1): `*_slack` is what that moves a sum by, zero when no point is unsafe.
"""

import numpy as np

import term_system_fn_model as FM
import term_system_mixed_model as MM
import term_system_nl_model as NM

EPS = NM.EPS
LOSSES = NM.LOSSES
SIZES = NM.SIZES  # 1, 255, 256, 257, 64 * 256 + 3
NL = NM.NL
U_G = NM.U_G
MAX_PARAMS = 8
SUM_TOL = 1e-6


def effective(coef, nl_params, param_values, coef_param, nl_param, exact=False):
    """(c_m, triples) the kernel computes with: stored * parameter where the index is >= 0, rounded to float32 once (exact=True: no
    rounding, every input taken as fp64 — the smooth function the finite differences are taken of)."""
    f = np.float64 if exact else np.float32
    coef = np.asarray(coef, dtype=f).copy()
    pv = None if param_values is None else np.asarray(param_values, dtype=f)
    for m, q in enumerate(coef_param if coef_param is not None else ()):
        if q >= 0:
            coef[m] = coef[m] * pv[q]
    nlp = None
    if nl_params is not None:
        nlp = np.asarray(nl_params, dtype=f).copy().reshape(-1, 3)
        for k, row in enumerate(nl_param if nl_param is not None else ()):
            for j, q in enumerate(row):
                if q >= 0:
                    nlp[k, j] = nlp[k, j] * pv[q]
    return coef.astype(np.float64), (None if nlp is None else nlp.astype(np.float64))


def _prep(dim, nt, nx, pair, jets, x, t, fn):
    N = jets[0].shape[1]
    nx = [tuple(v) + (0,) * (3 - len(v)) for v in nx]
    pair = [tuple(v) + (0,) * (3 - len(v)) for v in pair]
    jets = [None if j is None else np.asarray(j, dtype=np.float64) for j in jets]
    x = np.asarray(x, dtype=np.float64).reshape(N, dim)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    fn = None if fn is None else np.asarray(fn, dtype=np.float64).reshape(-1, N)
    return N, nx, pair, jets, x, t, fn


def _wbar(terms, coef, nonlinear, mask, nlv, value, rbar, rbar_bound, N):
    """Per masked k: [value, Bw, Bd, Rw] of the complete cotangent of w_k — sweep 2 of the sibling model for the nonlinear targets
    alone (the term summands in ascending m, then the pushes in descending k)."""
    wb = {k: [np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)] for k in mask}
    for m, (e, factors) in enumerate(terms):
        if not any(isinstance(f, str) and f in NL for f in factors):
            continue
        vals = [value(f) for f in factors]
        phi = [v for v, _ in vals]
        wide = [np.abs(v) + d for v, d in vals]
        for f, fac in enumerate(factors):
            if not (isinstance(fac, str) and fac in NL):
                continue
            others, oa, ow = coef[m] * np.ones(N), abs(coef[m]) * np.ones(N), abs(coef[m]) * np.ones(N)
            for g, (ph, wd) in enumerate(zip(phi, wide)):
                if g != f:
                    others, oa, ow = others * ph, oa * np.abs(ph), ow * wd
            acc = wb[NL[fac]]
            acc[0] = acc[0] + rbar[e] * others
            acc[1] = acc[1] + np.abs(rbar[e]) * ow
            acc[2] = acc[2] + np.abs(rbar[e]) * (ow - oa)
            acc[3] = acc[3] + rbar_bound[e] * ow
    for k in reversed(mask):
        src = nonlinear[k][1]
        if not isinstance(src, str):
            continue
        d, ed = nlv[k]["d"]
        dw = np.abs(d) + ed
        val, bw, bd, rw = wb[k]
        acc = wb[NL[src]]
        acc[0], acc[1], acc[2], acc[3] = acc[0] + val * d, acc[1] + bw * dw, acc[2] + bd * dw + bw * ed, acc[3] + rw * dw
    return wb


def evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn=None, nonlinear=(), nl_params=None, param_values=None,
             coef_param=None, nl_param=None, eq_weights=None, loss="mse", delta=1.0, grad_scale=1.0, residual_cotangent=None,
             exact=False):
    """Everything `pinn_term_residual_system_inv` returns, in fp64, with bounds: the keys of `term_system_nl_model.evaluate` on
    the effective values ("coef_sums" is G), and
      "eff_coef", "eff_nl"        the effective numbers;
      "wbar", "wbar_bound"        {k: (N,)} for the masked k;
      "H", "H_abs", "H_bound", "H_slack"   (K, 3): the sums, the sums of the absolute summands, of the per-point bounds, and what
                                  the unsafe points can move them by;  rows outside the mask and entries that are not formed: 0;
      "G_bound", "G_slack"        (T,): sum_n rbar_bound |prod|, and the same for the unsafe points;
      "param_grads", "param_abs", "param_bound", "param_slack"   (P,): the combination and its three tolerances' parts."""
    T = len(terms)
    nonlinear = [tuple(row[:2]) for row in nonlinear]
    K = len(nonlinear)
    P = 0 if param_values is None else len(param_values)
    coef_param = [-1] * T if coef_param is None else list(coef_param)
    nl_param = [(-1, -1, -1)] * K if nl_param is None else [tuple(r) for r in nl_param]
    assert P <= MAX_PARAMS and len(coef_param) == T and len(nl_param) == K
    assert all(-1 <= q < P for q in coef_param) and all(-1 <= q < P for r in nl_param for q in r)
    assert all(r[2] < 0 or nonlinear[k][0] == "pow" for k, r in enumerate(nl_param)), "a learnable exponent: pow only"
    ec, en = effective(coef, nl_params, param_values, coef_param, nl_param, exact)
    m = NM.evaluate(dim, nt, nx, pair, n_eq, terms, ec, jets, x, t, fn, nonlinear, en, eq_weights, loss, delta, grad_scale,
                    residual_cotangent)
    N, nxp, pairp, J, xx, tt, ff = _prep(dim, nt, nx, pair, jets, x, t, fn)
    mask = NM.mask_of(terms, nonlinear)
    nlv = NM._nl_values(mask, nonlinear, en, dim, nt, nxp, pairp, J, xx, tt)

    def value(fac):
        if isinstance(fac, str) and fac in NL:
            return nlv[NL[fac]]["w"]
        return FM._value(fac, dim, nt, nxp, pairp, J, xx, tt, ff)

    E = int(n_eq)
    w = np.ones(E) if eq_weights is None else np.asarray(eq_weights, dtype=np.float32).astype(np.float64)
    wb = _wbar(terms, ec, nonlinear, mask, nlv, value, m["rbar"], m["rbar_bound"], N)
    bad = m["unsafe"]
    if bad.any():  # what the unsafe points can move wbar by: the same sweep on the largest change of rbar, absolute values
        jump = (2.0 * abs(float(grad_scale)) * w * max(float(delta), 1.0))[:, None] * bad
        wj = _wbar(terms, ec, nonlinear, mask, nlv, value, jump, np.zeros((E, N)), N)
    cnt = m["count"]
    H, Ha, Hb, Hs = np.zeros((K, 3)), np.zeros((K, 3)), np.zeros((K, 3)), np.zeros((K, 3))
    wbar, wbar_bound, hpoint = {}, {}, {}
    for k in mask:
        op, src = nonlinear[k]
        shift, scale, p = (float(v) for v in en[k])
        assert scale != 0.0
        val, bw, bd, rw = wb[k]
        bnd = cnt * EPS * bw + bd + rw * (1.0 + cnt * EPS)
        wbar[k], wbar_bound[k] = val, bnd
        arg = nlv[k]["arg"]
        g1 = NM._g(op, arg, p)[1]
        es = nlv[k]["d"][1] / abs(scale)
        s, ds = nlv[NL[src]]["w"] if isinstance(src, str) else MM._value(src, dim, nt, nxp, pairp, J, xx, tt)
        ds = ds + np.zeros(N)
        wv, ew = nlv[k]["w"]
        h0 = val * g1
        b0 = np.abs(val) * es + bnd * (np.abs(g1) + es) + EPS * np.abs(h0)
        h1 = h0 * s
        b1 = b0 * (np.abs(s) + ds) + np.abs(h0) * ds + EPS * np.abs(h1)
        rows = [(h0, b0, np.abs(g1)), (h1, b1, np.abs(g1 * s))]
        if op == "pow":
            L = np.log(arg)
            darg = EPS * np.abs(arg) + abs(scale) * ds
            eL = U_G["log"] * EPS * np.abs(L) + darg / np.abs(arg)
            q = val * wv
            bq = np.abs(val) * ew + bnd * (np.abs(wv) + ew) + EPS * np.abs(q)
            h2 = q * L
            b2 = bq * (np.abs(L) + eL) + np.abs(q) * eL + EPS * np.abs(h2)
            rows.append((h2, b2, np.abs(wv * L)))
        hpoint[k] = [r[0] for r in rows]
        for j, (h, b, fac) in enumerate(rows):
            H[k, j], Ha[k, j], Hb[k, j] = h.sum(), np.abs(h).sum(), b.sum()
            if bad.any():
                Hs[k, j] = (wj[k][1] * fac).sum()
    prod = m["coef_prod"]
    Gb = np.asarray([(m["rbar_bound"][e] * np.abs(prod[i])).sum() for i, (e, _) in enumerate(terms)]) if T else np.zeros(0)
    Gs = np.zeros(T)
    if bad.any():
        Gs = np.asarray([(2.0 * abs(float(grad_scale)) * w[e] * max(float(delta), 1.0) * np.abs(prod[i][bad[e]])).sum()
                         for i, (e, _) in enumerate(terms)])
    sc = np.asarray(coef, dtype=np.float64)
    sn = None if nl_params is None else np.asarray(nl_params, dtype=np.float64).reshape(-1, 3)
    pg, pa, pb, ps = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    for i, q in enumerate(coef_param):
        if q >= 0:
            pg[q] += sc[i] * m["coef_sums"][i]
            pa[q] += abs(sc[i]) * m["coef_abs"][i]
            pb[q] += abs(sc[i]) * Gb[i]
            ps[q] += abs(sc[i]) * Gs[i]
    for k, row in enumerate(nl_param):
        for j, q in enumerate(row):
            if q >= 0 and k in mask:
                pg[q] += sn[k, j] * H[k, j]
                pa[q] += abs(sn[k, j]) * Ha[k, j]
                pb[q] += abs(sn[k, j]) * Hb[k, j]
                ps[q] += abs(sn[k, j]) * Hs[k, j]
    m.update({"eff_coef": ec, "eff_nl": en, "wbar": wbar, "wbar_bound": wbar_bound, "H": H, "H_abs": Ha, "H_bound": Hb, "H_slack": Hs,
              "H_point": hpoint, "G_bound": Gb, "G_slack": Gs, "param_grads": pg, "param_abs": pa, "param_bound": pb,
              "param_slack": ps, "mask": mask})
    return m


def pairing(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nonlinear, nl_params, param_values, coef_param, nl_param, rbar):
    """<rbar, r> in fp64 with NO rounding of the effective values: the smooth function of the parameters whose gradient
    `param_grads` is in the given-cotangent form."""
    m = evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nonlinear, nl_params, param_values, coef_param, nl_param,
                 residual_cotangent=rbar, exact=True)
    return float((np.asarray(rbar, dtype=np.float64) * m["r"]).sum())


def sums_fp32(dim, nt, nx, pair, terms, coef, jets, x, t, fn, nonlinear, nl_params, param_values, coef_param, nl_param, rbar):
    """(G (T,), H (K, 3)) of the given-cotangent form with every step of the header's recipe rounded to float32 in numpy, numpy's
    float32 functions standing for the device's, the summands added in double: what the number format alone does to the sums,
    without the code under test (`term_system_nl_model.coef_sums_fp32` for G; the same for wbar and the H products)."""
    f32 = np.float32
    ec, en = effective(coef, nl_params, param_values, coef_param, nl_param)
    G = NM.coef_sums_fp32(dim, nt, nx, pair, terms, jets, x, t, fn, nonlinear, en, rbar)
    C = len(nt)
    nxp = [tuple(v) + (0,) * (3 - len(v)) for v in nx]
    J = [None if j is None else np.asarray(j, dtype=f32) for j in jets]
    xs, ts = np.asarray(x, dtype=f32).reshape(-1, dim), np.asarray(t, dtype=f32).reshape(-1)
    N = ts.shape[0]
    rb = np.asarray(rbar, dtype=f32)
    fun = {"exp": np.exp, "log": np.log, "recip": lambda a: f32(1.0) / a, "sqrt": np.sqrt, "tanh": np.tanh, "sinh": np.sinh,
           "cosh": np.cosh, "sin": np.sin, "cos": np.cos}
    wk, sl, sv, ar = {}, {}, {}, {}

    def val(fac):
        if isinstance(fac, str):
            if fac in NL:
                return wk[NL[fac]]
            if fac in FM.FN:
                return np.asarray(fn, dtype=f32)[FM.FN[fac]]
            return ts if fac == "t" else xs[:, NM.COORDS[fac]]
        c, name = fac
        if name in NM.MIXED:
            k = NM.MIXED[name]
            (ba, ra), (bb, rb_) = NM.axis_row(c, NM.PAIRS[k][0], nt), NM.axis_row(c, NM.PAIRS[k][1], nt)
            return f32(0.5) * ((J[3 * C + 3 * c + k][2] - J[ba][ra]) - J[bb][rb_])
        if name in ("sin(u)", "cos(u)"):
            return (np.sin if name == "sin(u)" else np.cos)(J[3 * c][0])
        b, row = NM.M2.stream_of(name, nt[c], nxp[c])
        return J[3 * c + b][row]

    mask = NM.mask_of(terms, [tuple(r[:2]) for r in nonlinear])
    enf = None if en is None else en.astype(f32)
    for k in mask:
        op, src = nonlinear[k][:2]
        shift, scale, p = enf[k]
        s = val(src)
        arg = (np.float64(shift) + np.float64(scale) * s.astype(np.float64)).astype(f32)  # one rounding: the fma
        one = f32(1.0)
        if op == "pow":
            w = np.power(arg, p)
            slope = p * np.power(arg, p - one)
        else:
            w = fun[op](arg)
            slope = {"exp": lambda: w, "log": lambda: one / arg, "recip": lambda: -(w * w), "sqrt": lambda: f32(0.5) / w,
                     "tanh": lambda: one - w * w, "sinh": lambda: np.cosh(arg), "cosh": lambda: np.sinh(arg),
                     "sin": lambda: np.cos(arg), "cos": lambda: -np.sin(arg)}[op]()
        wk[k], sl[k], sv[k], ar[k] = w.astype(f32), slope.astype(f32), s, arg
    acc = {k: np.zeros(N, dtype=f32) for k in mask}
    for m, (e, factors) in enumerate(terms):
        phi = [val(f) for f in factors]
        hit = {}
        for f, fac in enumerate(factors):
            if isinstance(fac, str) and fac in NL:
                others = np.full(N, f32(ec[m]), dtype=f32)
                for g, ph in enumerate(phi):
                    if g != f:
                        others = others * ph
                hit[NL[fac]] = others if NL[fac] not in hit else hit[NL[fac]] + others
        for k, summ in hit.items():
            acc[k] = acc[k] + rb[e] * summ
    K = len(nonlinear)
    H = np.zeros((K, 3))
    for k in reversed(mask):
        src = nonlinear[k][1]
        scale = enf[k][1]
        if isinstance(src, str):
            acc[NL[src]] = acc[NL[src]] + acc[k] * (sl[k] * scale)
        h0 = acc[k] * sl[k]
        H[k, 0] = h0.astype(np.float64).sum()
        H[k, 1] = (h0 * sv[k]).astype(np.float64).sum()
        if nonlinear[k][0] == "pow":
            H[k, 2] = ((acc[k] * wk[k]) * np.log(ar[k])).astype(np.float64).sum()
    return G, H


# ---- the programs of tests/test_term_system_inv_kernel_gpu.py ---------------------------------------------------------------
# name: (base program of term_system_nl_model, its terms (None: the base's), param_values, coef_param, nl_param, the scales the
# stored numbers are divided by where learnable — the effective numbers stay the base's up to one rounding)
def _exp1():
    """One field, one EXP (the sibling's `bratu1d` with the shift 0.3, so that the shift's scale is not zero): the coefficient of
    the EXP term, and shift and scale of the EXP."""
    return "bratu1d", [("exp", (0, "u"), 0.3, 0.5, 1.0)], [0.8, 1.25, 0.5], [-1, -1, 0], [(2, 1, -1)]


def _euler1d():
    """`euler1d`: gamma behind two coefficients, the RECIP shift and the POW exponent learnable."""
    return "euler1d", None, [1.4, 2.0, 0.7], [-1, -1, -1, -1, -1, -1, -1, -1, 0, 0], [(1, -1, -1), (-1, -1, 2)]


def _caps8():
    """C = E = 4, dimension 3, 32 terms, 8 parameters: the sibling's `caps` chain with every "nl3" factor renamed "nl2", so that
    nl3 (SINH of nl2) is OUTSIDE the mask and carries a learnable shift (parameter 3) and NaN numbers that must never be read;
    parameter 0 is shared by three term coefficients and the scale of nl2; both shifts of the chain nl1(nl0(.)) are learnable
    (parameters 1, 2); parameter 7 is the scale of nl0; parameters 4 .. 6 sit behind one coefficient each."""
    cp = [-1] * 32
    cp[0] = cp[5] = cp[17] = 0
    cp[16], cp[20], cp[31] = 4, 5, 6
    return "caps", "nl3->nl2", [1.25, 0.8, 1.5, 2.0, 0.9, 1.1, 0.75, 1.6], cp, [(1, 7, -1), (2, -1, -1), (-1, 0, -1), (3, -1, -1)]


_SPECS = {"exp1": _exp1(), "euler1d": _euler1d(), "caps8": _caps8()}
PROGRAMS = {}
for _name, (_base, _edit, _pv, _cp, _np) in _SPECS.items():
    _dim, _nt, _nx, _pair, _neq, _terms, _coef, _K, _nl = NM.PROGRAMS[_base]
    if isinstance(_edit, list):
        _nl = _edit
    elif _edit:
        _terms = [(e, tuple("nl2" if f == "nl3" else f for f in fs)) for e, fs in _terms]
    PROGRAMS[_name] = (_dim, _nt, _nx, _pair, _neq, list(_terms), list(_coef), _K, list(_nl), list(_pv), list(_cp), [tuple(r) for r in _np])
EQ_WEIGHTS = {"exp1": NM.EQ_WEIGHTS["bratu1d"], "euler1d": NM.EQ_WEIGHTS["euler1d"], "caps8": NM.EQ_WEIGHTS["caps"]}
NAN_FUNCTIONS = {"caps8": (3,)}  # nonlinear functions outside the mask: NaN numbers on the device, never read

# (program, size) whose default seed leaves more than 1 % of the points within their bound of a kink of l', or whose float32
# evaluation in numpy alone (`sums_fp32`) leaves half of the sums' 1e-6: the next seed that does neither
# (tests/test_term_system_inv_cpu.py checks both on the model alone)
_SEED_SHIFT = {}


def inputs(name, N, seed=None):
    """Standard-normal jets, coordinates, function rows and (E, N) cotangent in fp32, seeded per (program, size); the stored
    coefficients and triples are the base program's numbers divided by the parameter where learnable."""
    dim, nt, nx, pair, n_eq, terms, coef, K, nl, pv, cp, npar = PROGRAMS[name]
    if seed is None:
        seed = 41000 + 1000 * sorted(PROGRAMS).index(name) + N + _SEED_SHIFT.get((name, N), 0)
    rng = np.random.default_rng(seed)
    jets = [None if s is None else rng.standard_normal(s).astype(np.float32) for s in NM.block_shapes(dim, nt, nx, pair, N)]
    x = rng.standard_normal((N, dim)).astype(np.float32)
    t = rng.standard_normal(N).astype(np.float32)
    rbar = rng.standard_normal((n_eq, N)).astype(np.float32)
    fn = rng.standard_normal((K, N)).astype(np.float32)
    pv = np.asarray(pv, dtype=np.float32)
    coef = np.asarray([c / float(pv[q]) if q >= 0 else c for c, q in zip(coef, cp)], dtype=np.float32)
    params = np.asarray([row[2:] for row in nl], dtype=np.float64).reshape(len(nl), 3)
    for k, row in enumerate(npar):
        for j, q in enumerate(row):
            if q >= 0:
                params[k, j] /= float(pv[q])
    params = params.astype(np.float32)
    for k in NAN_FUNCTIONS.get(name, ()):
        params[k] = np.nan
    return (dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, [row[:2] for row in nl], params, pv, cp, npar)


engine_terms = NM.engine_terms
engine_nonlinear = NM.engine_nonlinear
