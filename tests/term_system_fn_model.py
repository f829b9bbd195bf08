"""fp64 specification of `pinn_term_residual_system_fn` (include/pinn_jet.h) in numpy, with per-point error bounds.

A program is (dimension, nt, nx, pair, n_equations, terms, coefficients, n_functions): tests/term_system_mixed_model.py's
programs plus the number K of known functions and the factor names "fn0" .. "fn3", given like a coordinate (a string, no
field).  The function values are a (K, N) array, row k the fp32 values of g_k at the points.

A function value is one more exactly known fp32 factor among the at most four of a product, exactly as a coordinate is: it
enters the products of sweep 1, of the other factors' derivative summands and of the coefficient sums, it has no error of its
own (d = 0) and it is no cotangent target.  The count of roundings of a product does not change, so the bound formulas of
tests/term_system_mixed_model.py apply unchanged: `evaluate` below is that model's `evaluate` with the one more kind of factor
value.  With no function factor in the program its outputs are identical to that model's, whatever the function rows hold
(tests/test_term_system_fn_cpu.py checks it).

The sums over the points are compared as the sibling's are, to 1e-6 of the sum of the absolute summands.
"""

import numpy as np

import term_nd_model as M2
import term_pde_model as M1
import term_system_mixed_model as MM

EPS = MM.EPS
COORDS = MM.COORDS
LOSSES = MM.LOSSES
SIZES = MM.SIZES  # 1, 255, 256, 257, 64 * 256 + 3
PAIRS = MM.PAIRS
MIXED = MM.MIXED
D2 = MM.D2
MAX_FUNCTIONS = 4
FN = {f"fn{k}": k for k in range(MAX_FUNCTIONS)}

axis_row = MM.axis_row
block_shapes = MM.block_shapes


def _value(fac, dim, nt, nx, pair, jets, x, t, fn):
    """(value, absolute error of the fp32 value against it): the sibling's, and row k of the function values for "fn<k>"."""
    if isinstance(fac, str) and fac in FN:
        assert fn is not None and FN[fac] < fn.shape[0], (fac, None if fn is None else fn.shape)
        return fn[FN[fac]], 0.0
    return MM._value(fac, dim, nt, nx, pair, jets, x, t)


def evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn=None, eq_weights=None, loss="mse", delta=1.0, grad_scale=1.0,
             residual_cotangent=None):
    """Everything `pinn_term_residual_system_fn` returns, in fp64, with bounds: the keys of `term_system_mixed_model.evaluate`.
    fn: the (K, N) function values (None with K = 0); only the rows that a term names are read."""
    C, E, T = len(nt), int(n_eq), len(terms)
    N = jets[0].shape[1]
    nx = [tuple(v) + (0,) * (3 - len(v)) for v in nx]
    pair = [tuple(v) + (0,) * (3 - len(v)) for v in pair]
    coef = np.asarray(coef, dtype=np.float64)
    w = np.ones(E) if eq_weights is None else np.asarray(eq_weights, dtype=np.float32).astype(np.float64)
    shapes = block_shapes(dim, nt, nx, pair, N)
    jets = [None if j is None else np.asarray(j, dtype=np.float64) for j in jets]
    assert len(jets) == 6 * C
    for b, s in enumerate(shapes):
        assert (jets[b] is None) == (s is None) and (s is None or jets[b].shape == s), (b, s)
    x = np.asarray(x, dtype=np.float64).reshape(N, dim)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    if fn is not None:
        fn = np.asarray(fn, dtype=np.float64).reshape(-1, N)
    F = max([len(f) for _, f in terms] + [0])
    T_e = [sum(1 for e, _ in terms if e == k) for k in range(E)]

    r, A, Ed = np.zeros((E, N)), np.zeros((E, N)), np.zeros((E, N))
    prod_all = np.ones((T, N))
    summands = []  # per term: list of (block, row, value, |.| on the widened factors, the same minus |.| on the exact ones)
    for m, (e, factors) in enumerate(terms):
        vals = [_value(f, dim, nt, nx, pair, jets, x, t, fn) for f in factors]
        phi = [v for v, _ in vals]
        wide = [np.abs(v) + d for v, d in vals]
        p, pa, pw = np.ones(N), np.ones(N), np.ones(N)
        for ph, wd in zip(phi, wide):
            p, pa, pw = p * ph, pa * np.abs(ph), pw * wd
        prod_all[m] = p
        r[e] += coef[m] * p
        A[e] += abs(coef[m]) * pw
        Ed[e] += abs(coef[m]) * (pw - pa)
        mine = []
        for f, fac in enumerate(factors):
            if isinstance(fac, str):
                continue  # a coordinate or a known function: no derivative summand
            c, name = fac
            others, oa, ow = coef[m] * np.ones(N), abs(coef[m]) * np.ones(N), abs(coef[m]) * np.ones(N)
            for g, (ph, wd) in enumerate(zip(phi, wide)):
                if g != f:
                    others, oa, ow = others * ph, oa * np.abs(ph), ow * wd
            u = jets[3 * c][0]
            if name == "sin(u)":
                (b, s), term, scale = (3 * c, 0), others * np.cos(u), np.abs(np.cos(u))
            elif name == "cos(u)":
                (b, s), term, scale = (3 * c, 0), -others * np.sin(u), np.abs(np.sin(u))
            elif name in MIXED:  # g_k is collected in row 2 of the P block; the write-out below spreads it
                (b, s), term, scale = (3 * C + 3 * c + MIXED[name], 2), others, 1.0
            else:
                (a, s), term, scale = M2.stream_of(name, nt[c], nx[c]), others, 1.0
                b = 3 * c + a
            mine.append((b, s, term, ow * scale, (ow - oa) * scale))
        summands.append(mine)
    r_bound = np.stack([(T_e[e] + F + 2) * EPS * A[e] + Ed[e] for e in range(E)])

    lv, slope = M1.loss_and_slope(r, loss, delta)
    if residual_cotangent is not None:
        rbar = np.asarray(residual_cotangent, dtype=np.float64).reshape(E, N)
        rbar_bound = np.zeros((E, N))
        unsafe = np.zeros((E, N), dtype=bool)
    else:
        gw = float(grad_scale) * w  # the device rounds this product to fp32 once: inside the 2 EPS |rbar| below
        rbar = gw[:, None] * slope
        if loss == "mae":
            rbar_bound = np.zeros((E, N))
            unsafe = np.abs(r) <= r_bound
        elif loss == "huber":
            rbar_bound = np.where(np.abs(r) < delta, np.abs(gw)[:, None] * r_bound, 0.0)
            unsafe = np.abs(np.abs(r) - delta) <= r_bound
        else:
            rbar_bound = 2.0 * np.abs(gw)[:, None] * r_bound
            unsafe = np.zeros((E, N), dtype=bool)
        rbar_bound = rbar_bound + 2 * EPS * np.abs(rbar)

    def zeros():
        return [None if s is None else np.zeros(s) for s in shapes]

    cot, Bw, Bd, Rw = zeros(), zeros(), zeros(), zeros()
    touched = [None if s is None else np.zeros(s[0], dtype=bool) for s in shapes]
    for m, (e, _) in enumerate(terms):
        for b, s, term, aw, ad in summands[m]:
            cot[b][s] += rbar[e] * term
            Bw[b][s] += np.abs(rbar[e]) * aw
            Bd[b][s] += np.abs(rbar[e]) * ad
            Rw[b][s] += rbar_bound[e] * aw
            touched[b][s] = True
    count_c = T + F + 5
    cot_bound = [None if s is None else count_c * EPS * bw + bd + rw * (1.0 + count_c * EPS)
                 for s, bw, bd, rw in zip(shapes, Bw, Bd, Rw)]
    # the write-out: per field, in ascending pair index
    for c in range(C):
        for k in range(3):
            pb = 3 * C + 3 * c + k
            if pair[c][k] != 2 or not touched[pb][2]:
                continue  # g is exactly zero: p_k = 0 and the axis rows keep their bits
            cot[pb][2] *= 0.5
            cot_bound[pb][2] *= 0.5
            for a in PAIRS[k]:
                b, s = axis_row(c, a, nt)
                cot[b][s] -= cot[pb][2]
                cot_bound[b][s] += cot_bound[pb][2]
                cot_bound[b][s] += EPS * (np.abs(cot[b][s]) + cot_bound[b][s])
                touched[b][s] = True

    eq_loss = lv.sum(1)
    eq_abs = np.abs(lv).sum(1)
    coef_summands = np.stack([rbar[e] * prod_all[m] for m, (e, _) in enumerate(terms)]) if T else np.zeros((0, N))
    return {"r": r, "r_bound": r_bound, "eq_loss": eq_loss, "eq_abs": eq_abs, "loss_sum": float((w * eq_loss).sum()),
            "loss_abs": float((w * eq_abs).sum()), "rbar": rbar, "rbar_bound": rbar_bound, "cot": cot, "cot_bound": cot_bound,
            "touched": touched, "coef_sums": coef_summands.sum(1), "coef_abs": np.abs(coef_summands).sum(1), "coef_prod": prod_all,
            "unsafe": unsafe, "count": count_c}


# ---- the programs of tests/test_term_system_fn_kernel_gpu.py ---------------------------------------------------------------
def _u(c, name="u"):
    return (c, name)


def _source1d():
    """(a) C = 1 in 1-D, u_t - g u_xx - f = 0: a variable coefficient times a stream, and a term that is a source alone."""
    terms = [(0, (_u(0, "u_t"),)), (0, ("fn0", _u(0, "u_xx"))), (0, ("fn1",))]
    return 1, (1,), ((2, 0, 0),), ((0, 0, 0),), 1, terms, [1.0, -0.7, -1.0], 2


def _elasticity_force(mu=0.5):
    """(b) 2-D elasticity with a variable modulus a(x, y) = fn2 multiplying the grad-div terms (the mixed factors among them)
    and a body force per equation (fn0, fn1)."""
    u, v = 0, 1
    terms = [(0, (_u(u, "u_t"),)), (0, (_u(u, "u_xx"),)), (0, (_u(u, "u_yy"),)), (0, ("fn2", _u(u, "u_xx"))),
             (0, ("fn2", _u(v, "u_xy"))), (0, ("fn0",)),
             (1, (_u(v, "u_t"),)), (1, (_u(v, "u_xx"),)), (1, (_u(v, "u_yy"),)), (1, (_u(u, "u_xy"), "fn2")),
             (1, ("fn2", _u(v, "u_yy"))), (1, ("fn1",))]
    coef = [1.0, -mu, -mu, -1.0, -1.0, -1.0, 1.0, -mu, -mu, -1.0, -1.0, -1.0]
    return 2, (1, 1), ((2, 2, 0), (2, 2, 0)), ((2, 0, 0), (2, 0, 0)), 2, terms, coef, 3


def _caps():
    """(c) The sibling's caps (C = E = 4, dimension 3, 32 terms, the LDS maximum) with its terms 8 .. 15 replaced by terms that
    name all four functions: one function twice in a term, function x trig x coordinate, a function beside a mixed factor, a
    term of functions only."""
    dim, nt, nx, pair, n_eq, terms, coef = MM.PROGRAMS["caps"]
    mine = [
        (0, ("fn0", "fn0", _u(0, "u_xx"))),                       # one function twice in a term
        (1, ("fn1", _u(1, "sin(u)"), "x")),                       # function x trig x coordinate
        (2, ("fn2", _u(2, "cos(u)"), "t", _u(3, "u_y"))),
        (3, ("fn3", _u(3, "u_xy"), _u(3, "u_xy"))),               # a function beside the same mixed factor twice
        (0, ("fn0", "fn1", "fn2", "fn3")),                        # functions only: no cotangent at all
        (1, (_u(0, "u_yz"), "fn3", _u(1, "u_zz"), "fn1")),
        (2, ("fn2",)),                                            # a source alone
        (3, (_u(2), "fn0", _u(2), "z")),
    ]
    terms = list(terms[:8]) + mine + list(terms[16:])
    assert len(terms) == 32
    return dim, nt, nx, pair, n_eq, terms, coef, 4


def _one_named():
    """(d) n_functions = 4 with only function 2 named (the sibling's `one_pair` plus two terms): the rows 0, 1 and 3 of
    fn_values are filled with NaN and must never be read."""
    dim, nt, nx, pair, n_eq, terms, coef = MM.PROGRAMS["one_pair"]
    terms = list(terms) + [(0, ("fn2", _u(0, "u_x"))), (1, ("fn2", "fn2", _u(1, "u_xz")))]
    return dim, nt, nx, pair, n_eq, terms, list(coef) + [0.8, -0.35], 4


PROGRAMS = {"source1d": _source1d(), "elasticity_force": _elasticity_force(), "caps": _caps(), "one_named": _one_named()}
EQ_WEIGHTS = {"source1d": (1.5,), "elasticity_force": (1.0, 2.0), "caps": MM.EQ_WEIGHTS["caps"], "one_named": (1.0, 0.5)}
NAN_ROWS = {"one_named": (0, 1, 3)}  # rows of fn_values that no term names: NaN on the device, never read

# (program, size) whose default seed puts more than 1 % of the points within their bound of a kink of l' (checked on the model
# alone in tests/test_term_system_fn_cpu.py): the next seed is taken
_SEED_SHIFT = {}


def inputs(name, N, seed=None):
    """Standard-normal jets, coordinates and function rows in fp32, the program's coefficients and a standard-normal (E, N)
    cotangent, seeded per (program, size).  The rows of `NAN_ROWS` are NaN."""
    dim, nt, nx, pair, n_eq, terms, coef, K = PROGRAMS[name]
    if seed is None:
        seed = 23000 + 1000 * sorted(PROGRAMS).index(name) + N + _SEED_SHIFT.get((name, N), 0)
    rng = np.random.default_rng(seed)
    jets = [None if s is None else rng.standard_normal(s).astype(np.float32) for s in block_shapes(dim, nt, nx, pair, N)]
    x = rng.standard_normal((N, dim)).astype(np.float32)
    t = rng.standard_normal(N).astype(np.float32)
    rbar = rng.standard_normal((n_eq, N)).astype(np.float32)
    fn = rng.standard_normal((K, N)).astype(np.float32)
    for k in NAN_ROWS.get(name, ()):
        fn[k] = np.nan
    return dim, nt, nx, pair, n_eq, terms, np.asarray(coef, dtype=np.float32), jets, x, t, rbar, fn


def engine_terms(terms):
    """(factors per term, equation_of) in the form `engine.FnSystemTermDesc` takes."""
    return [f for _, f in terms], [e for e, _ in terms]
