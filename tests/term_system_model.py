"""fp64 specification of `pinn_term_residual_system` (include/pinn_jet.h) in numpy, with per-point error bounds.

A program is (dimension, nt, nx, n_equations, terms, coefficients): nt[c] and nx[c] = (nx0, nx1, nx2) per field, terms a list of
(equation, factors) in ascending term index, a factor being a coordinate name ("x", "y", "z", "t") or (field, name) with the
name one of tests/term_nd_model.py's stream / trig names.  The inputs are the fp32 numbers the kernel reads, widened to fp64:
the coefficients, the 3 C blocks of jets (entry 3 c + a; block (c, 0): (1 + nt_c + nx0_c, N), block (c, a >= 1): (1 + nx_a, N)
or None; row 0 of a block with a >= 1 is never read), x (N, dimension), t (N,), the equation weights.

The bounds follow the summation order the header states, by the argument of tests/term_pde_model.py (every count of half-ulp
roundings is doubled to cover fused multiply-adds, the device's sin / cos and the order of the adds).

Sweep 1.  r_e adds the T_e terms of equation e in ascending m, each product rounding at most F times (F = the largest factor
count), plus 2 for a sin / cos factor: |r_e(fp32) - r_e| <= (T_e + F + 2) 2^-23 A_e, A_e = sum_{m in e} |c_m| prod_f |phi_{m,f}|.

rbar_e = fl(fl(grad_scale omega_e) l'(r_e)): two roundings (2 2^-23 |rbar_e| after doubling) on top of what r_e's error does
to l' (nothing for mae away from the kink, |gs omega_e| r_bound on Huber's quadratic branch, twice that for mse).

Sweep 2.  The accumulator of (field, stream) receives, in ascending m, fl(rbar_e(m) S_m) with S_m the sum of the at most four
derivative summands of term m that belong to it.  A summand is a product of at most F numbers (F roundings, 2 more under a
trig factor: the cos / sin it is multiplied with), S_m adds at most 4 of them (3 roundings), the product with rbar is one
more, and the T terms are added with at most T - 1 roundings, each relative to a partial sum that never exceeds
B = sum_m |rbar_e(m)| sum |summand| in magnitude: (T + F + 5) half-ulps, doubled: (T + F + 5) 2^-23 B.  To that the error of
rbar itself is added: sum_m rbar_bound_e(m) sum |summand| (and its second-order product with the first part).

The sums over the points are accumulated in double from fp32 summands: the tests compare them with the fp64 sums to 1e-6 of
the sum of the absolute summands, as the sibling kernels' tests do.
"""

import numpy as np

import term_nd_model as M2
import term_pde_model as M1

EPS = M1.EPS
COORDS = {"x": 0, "y": 1, "z": 2}
LOSSES = M1.LOSSES
SIZES = (1, 255, 256, 257, 64 * 256 + 3)


def block_shapes(dim, nt, nx, N):
    """Shapes of the 3 C blocks (None where a block does not exist)."""
    out = []
    for c in range(len(nt)):
        out.append((1 + nt[c] + nx[c][0], N))
        out += [(1 + nx[c][a], N) if (a < dim and nx[c][a] > 0) else None for a in (1, 2)]
    return out


def _value(fac, dim, nt, nx, jets, x, t):
    if isinstance(fac, str):
        return t if fac == "t" else x[:, COORDS[fac]]
    c, name = fac
    u = jets[3 * c][0]
    if name == "sin(u)":
        return np.sin(u)
    if name == "cos(u)":
        return np.cos(u)
    b, row = M2.stream_of(name, nt[c], nx[c])
    return jets[3 * c + b][row]


def evaluate(dim, nt, nx, n_eq, terms, coef, jets, x, t, eq_weights=None, loss="mse", delta=1.0, grad_scale=1.0,
             residual_cotangent=None):
    """Everything `pinn_term_residual_system` returns, in fp64, with bounds.

    r, r_bound            (E, N) residuals and their fp32 error bounds
    eq_loss, eq_abs       (E,): sum_n l(r_e,n) and the sum of the absolute summands
    loss_sum, loss_abs    sum_e omega_e eq_loss[e] and the same of the absolute summands
    rbar, rbar_bound      (E, N)
    cot, cot_bound        lists of 3 C blocks (None where the block does not exist)
    touched               list of 3 C boolean (rows,) arrays: the rows some term's derivative goes to; every other row of a
                          cotangent block must be exactly zero
    coef_sums, coef_abs   (T,);  coef_prod (T, N): prod_f phi_{m,f}
    unsafe                (E, N) bool: |r_e| within its bound of the kink of l'
    residual_cotangent: (E, N) when given.
    """
    C, E, T = len(nt), int(n_eq), len(terms)
    N = jets[0].shape[1]
    nx = [tuple(v) + (0,) * (3 - len(v)) for v in nx]
    coef = np.asarray(coef, dtype=np.float64)
    w = np.ones(E) if eq_weights is None else np.asarray(eq_weights, dtype=np.float32).astype(np.float64)
    shapes = block_shapes(dim, nt, nx, N)
    jets = [None if j is None else np.asarray(j, dtype=np.float64) for j in jets]
    assert len(jets) == 3 * C
    for b, s in enumerate(shapes):
        assert (jets[b] is None) == (s is None) and (s is None or jets[b].shape == s), (b, s)
    x = np.asarray(x, dtype=np.float64).reshape(N, dim)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    F = max([len(f) for _, f in terms] + [0])
    T_e = [sum(1 for e, _ in terms if e == k) for k in range(E)]

    r, A = np.zeros((E, N)), np.zeros((E, N))
    prod_all = np.ones((T, N))
    summands = []  # per term: list of (block, row, values)
    for m, (e, factors) in enumerate(terms):
        phi = [_value(f, dim, nt, nx, jets, x, t) for f in factors]
        p = np.ones(N)
        for ph in phi:
            p = p * ph
        prod_all[m] = p
        r[e] += coef[m] * p
        A[e] += abs(coef[m]) * np.abs(p)
        mine = []
        for f, fac in enumerate(factors):
            if isinstance(fac, str):
                continue
            c, name = fac
            others = coef[m] * np.ones(N)
            for g, ph in enumerate(phi):
                if g != f:
                    others = others * ph
            u = jets[3 * c][0]
            if name == "sin(u)":
                (b, s), term = (0, 0), others * np.cos(u)
            elif name == "cos(u)":
                (b, s), term = (0, 0), -others * np.sin(u)
            else:
                (b, s), term = M2.stream_of(name, nt[c], nx[c]), others
            mine.append((3 * c + b, s, term))
        summands.append(mine)
    r_bound = np.stack([(T_e[e] + F + 2) * EPS * A[e] for e in range(E)])

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

    cot = [None if s is None else np.zeros(s) for s in shapes]
    B = [None if s is None else np.zeros(s) for s in shapes]       # sum_m |rbar| sum |summand|
    Rb = [None if s is None else np.zeros(s) for s in shapes]      # sum_m rbar_bound sum |summand|
    touched = [None if s is None else np.zeros(s[0], dtype=bool) for s in shapes]
    for m, (e, _) in enumerate(terms):
        for b, s, term in summands[m]:
            cot[b][s] += rbar[e] * term
            B[b][s] += np.abs(rbar[e]) * np.abs(term)
            Rb[b][s] += rbar_bound[e] * np.abs(term)
            touched[b][s] = True
    count_c = T + F + 5
    cot_bound = [None if s is None else count_c * EPS * bb + rb * (1.0 + count_c * EPS) for s, bb, rb in zip(shapes, B, Rb)]

    eq_loss = lv.sum(1)
    eq_abs = np.abs(lv).sum(1)
    coef_summands = np.stack([rbar[e] * prod_all[m] for m, (e, _) in enumerate(terms)]) if T else np.zeros((0, N))
    return {"r": r, "r_bound": r_bound, "eq_loss": eq_loss, "eq_abs": eq_abs, "loss_sum": float((w * eq_loss).sum()),
            "loss_abs": float((w * eq_abs).sum()), "rbar": rbar, "rbar_bound": rbar_bound, "cot": cot, "cot_bound": cot_bound,
            "touched": touched, "coef_sums": coef_summands.sum(1), "coef_abs": np.abs(coef_summands).sum(1), "coef_prod": prod_all,
            "unsafe": unsafe, "count": count_c}


# ---- the programs of tests/test_term_system_kernel_gpu.py ------------------------------------------------------------------
def _u(c, name="u"):
    return (c, name)


def _gray_scott():
    """u_t - Du u_xx + u v v - F + F u;  v_t - Dv v_xx - u v v + (F + k) v: a term without factors, the cross-field product."""
    u, v = 0, 1
    terms = [(0, (_u(u, "u_t"),)), (0, (_u(u, "u_xx"),)), (0, (_u(u), _u(v), _u(v))), (0, ()), (0, (_u(u),)),
             (1, (_u(v, "u_t"),)), (1, (_u(v, "u_xx"),)), (1, (_u(u), _u(v), _u(v))), (1, (_u(v),))]
    coef = [1.0, -0.16, 1.0, -0.035, 0.035, 1.0, -0.08, -1.0, 0.1]
    return 1, (1, 1), ((2, 0, 0), (2, 0, 0)), 2, terms, coef


def _navier_stokes(nu=0.1):
    """2-D incompressible Navier-Stokes in (u, v, p): two momentum equations of six terms and continuity, 14 terms.  The
    pressure's streams p_x, p_y sit in the set (1, 1) on axis 0 (the smallest compiled set that holds order 1 along x)."""
    u, v, p = 0, 1, 2
    terms = [(0, (_u(u, "u_t"),)), (0, (_u(u), _u(u, "u_x"))), (0, (_u(v), _u(u, "u_y"))), (0, (_u(p, "u_x"),)),
             (0, (_u(u, "u_xx"),)), (0, (_u(u, "u_yy"),)),
             (1, (_u(v, "u_t"),)), (1, (_u(u), _u(v, "u_x"))), (1, (_u(v), _u(v, "u_y"))), (1, (_u(p, "u_y"),)),
             (1, (_u(v, "u_xx"),)), (1, (_u(v, "u_yy"),)),
             (2, (_u(u, "u_x"),)), (2, (_u(v, "u_y"),))]
    coef = [1.0, 1.0, 1.0, 1.0, -nu, -nu, 1.0, 1.0, 1.0, 1.0, -nu, -nu, 1.0, 1.0]
    return 2, (1, 1, 1), ((2, 2, 0), (2, 2, 0), (1, 1, 0)), 3, terms, coef


def _caps():
    """The caps: C = E = 4, dimension 3, 32 terms of 4 factors each; trig and coordinate factors; terms whose summands share
    an accumulator (u u sin(u) cos(u)), terms across all four fields; the rest is drawn from every field's streams with a fixed seed."""
    nt = (2, 1, 1, 2)
    nx = ((2, 2, 2), (4, 1, 1), (2, 2, 2), (0, 2, 1))
    names = []
    for c in range(4):
        have = ["u", "sin(u)", "cos(u)"] + ["u_t", "u_tt"][: nt[c]] + ["u_x", "u_xx", "u_xxx", "u_xxxx"][: nx[c][0]]
        have += ["u_y", "u_yy"][: nx[c][1]] + ["u_z", "u_zz"][: nx[c][2]]
        names.append(have)
    fixed = [
        (0, (_u(0), _u(0), _u(0, "sin(u)"), _u(0, "cos(u)"))),          # four summands into one accumulator
        (1, (_u(0), _u(1), _u(2), _u(3))),                              # one factor of every field
        (2, ("x", "y", "z", "t")),                                      # coordinates only: no cotangent at all
        (3, (_u(3, "u_tt"), _u(3, "u_yy"), _u(3, "u_z"), "t")),
        (0, (_u(1, "u_xxxx"), _u(1, "u_xxx"), _u(1, "u_y"), _u(1, "u_z"))),
        (1, (_u(2, "u_zz"), _u(2, "u_zz"), "x", _u(2, "cos(u)"))),      # a repeated stream: two summands into one accumulator
        (2, (_u(0, "u_tt"), _u(0, "u_yy"), _u(0, "u_zz"), "z")),
        (3, (_u(3, "sin(u)"), _u(3, "sin(u)"), _u(2, "u_t"), "y")),
    ]
    rng = np.random.default_rng(20240)
    terms = list(fixed)
    while len(terms) < 32:
        factors = []
        for _ in range(4):
            k = int(rng.integers(0, 10))
            if k == 0:
                factors.append(["x", "y", "z", "t"][int(rng.integers(0, 4))])
            else:
                c = int(rng.integers(0, 4))
                factors.append((c, names[c][int(rng.integers(0, len(names[c])))]))
        terms.append((len(terms) % 4, tuple(factors)))
    coef = [float(v) for v in np.round(rng.uniform(0.2, 1.2, 32) * rng.choice([-1.0, 1.0], 32), 3)]
    return 3, nt, nx, 4, terms, coef


def _unnamed_field():
    """Three fields, two equations, dimension 2; no term names field 1, whose two blocks must come back all zero."""
    terms = [(0, (_u(0, "u_t"),)), (0, (_u(0, "u_xx"),)), (0, (_u(0, "u_yy"),)), (0, (_u(2), _u(0))),
             (1, (_u(2, "u_t"),)), (1, (_u(2, "u_x"), _u(0, "u_y"))), (1, ("x", _u(2, "sin(u)")))]
    coef = [1.0, -0.1, -0.1, 0.5, 1.0, 0.75, -0.3]
    return 2, (1, 1, 1), ((2, 2, 0), (1, 2, 0), (1, 0, 0)), 2, terms, coef


PROGRAMS = {"gray_scott": _gray_scott(), "navier_stokes": _navier_stokes(), "caps": _caps(), "unnamed_field": _unnamed_field()}
EQ_WEIGHTS = {"gray_scott": (1.0, 2.0), "navier_stokes": (1.0, 1.0, 4.0), "caps": (1.0, 0.5, 0.25, 2.0), "unnamed_field": (1.0, 0.0)}

# (program, size) whose default seed puts a point within its bound of a kink of l' (tests/test_term_system_cpu.py checks that
# at most 1 % of the points are): the next seed is taken
_SEED_SHIFT = {}


def inputs(name, N, seed=None):
    """Standard-normal jets and coordinates in fp32, the program's coefficients and a standard-normal (E, N) cotangent, seeded
    per (program, size)."""
    dim, nt, nx, n_eq, terms, coef = PROGRAMS[name]
    if seed is None:
        seed = 9000 + 1000 * sorted(PROGRAMS).index(name) + N + _SEED_SHIFT.get((name, N), 0)
    rng = np.random.default_rng(seed)
    jets = [None if s is None else rng.standard_normal(s).astype(np.float32) for s in block_shapes(dim, nt, nx, N)]
    x = rng.standard_normal((N, dim)).astype(np.float32)
    t = rng.standard_normal(N).astype(np.float32)
    rbar = rng.standard_normal((n_eq, N)).astype(np.float32)
    return dim, nt, nx, n_eq, terms, np.asarray(coef, dtype=np.float32), jets, x, t, rbar


def engine_terms(terms):
    """(factors per term, equation_of) in the form `engine.SystemTermDesc` takes."""
    return [f for _, f in terms], [e for e, _ in terms]
