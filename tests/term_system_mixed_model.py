"""fp64 specification of `pinn_term_residual_system_mixed` (include/pinn_jet.h) in numpy, with per-point error bounds.

A program is (dimension, nt, nx, pair, n_equations, terms, coefficients): tests/term_system_model.py's programs plus pair[c] =
the order 0 or 2 of the pairs (x,y), (x,z), (y,z) of field c, and the factor names "u_xy", "u_xz", "u_yz" of a field.  The jets
are 6 C blocks: entry 3 c + a the axis block (c, a) as there, entry 3 C + 3 c + k the (3, N) block of field c's launch along
e_a + e_b (only its row 2, P_2, is read), None where pair[c][k] is 0.

    u_ab = 0.5 ((P_2 - A_2) - B_2),   A_2, B_2 the order-2 rows of the field's two axis blocks (axis 0: row nt_c + 2).

The bounds extend the argument of tests/term_system_model.py by the roundings the header states, counted as
tests/term_mixed_model.py counts them.  u_ab takes two fp32 roundings (the two subtractions; the product with 0.5 is exact), each
at most 2^-24 of a partial result no larger than |P_2| + |A_2| + |B_2|: the fp32 value is within d = D2 EPS (|P_2| + |A_2| +
|B_2|) / 2 of the fp64 one, D2 = 2, EPS = 2^-23.  A factor that is off by d enters a product as |phi| + d at most, so

Sweep 1:  |r_e(fp32) - r_e| <= (T_e + F + 2) EPS sum_{m in e} |c_m| prod_f (|phi| + d)  +  sum_{m in e} |c_m| (prod_f (|phi| + d)
          - prod_f |phi|): the sibling's bound on the widened absolute sum, plus what the factor errors move.
Sweep 2:  the accumulator of a (field, stream) target — u_ab of a field is a target of its own — is within
          (T + F + 5) EPS Bw + Bd + Rw (1 + (T + F + 5) EPS) of the fp64 one, Bw = sum_m |rbar| sum |summand| on the widened
          factors, Bd = the same on the widened minus the exact factors, Rw = sum_m rbar_bound sum |summand| (widened).
Write-out, per field in ascending pair index: p_k = g_k / 2 is exact and goes to row 2 of the P block with half the bound of
          g_k; each of the two axis rows has p_k subtracted: its bound grows by that of p_k and by one rounding, EPS of the
          row's new value (and of its bound).  An axis row gains one such subtraction per pair that touches it.
With every pair order 0 there is no d and no write-out step: values and bounds are tests/term_system_model.py's.

The sums over the points are compared as the sibling's are, to 1e-6 of the sum of the absolute summands.
"""

import numpy as np

import term_nd_model as M2
import term_pde_model as M1
import term_system_model as SM

EPS = M1.EPS
COORDS = SM.COORDS
LOSSES = SM.LOSSES
SIZES = SM.SIZES  # a lone point, a partial wave, the block edge, one past it, a second grid-stride round with a ragged tail
PAIRS = ((0, 1), (0, 2), (1, 2))
MIXED = {"u_xy": 0, "u_xz": 1, "u_yz": 2}
D2 = 2


def axis_row(c, a, nt):
    """(block, row) of the order-2 derivative of field c along axis a."""
    return (3 * c, nt[c] + 2) if a == 0 else (3 * c + a, 2)


def block_shapes(dim, nt, nx, pair, N):
    """Shapes of the 6 C blocks (None where a block does not exist)."""
    C = len(nt)
    return SM.block_shapes(dim, nt, nx, N) + [(3, N) if pair[c][k] == 2 else None for c in range(C) for k in range(3)]


def _value(fac, dim, nt, nx, pair, jets, x, t):
    """(value, absolute error of the fp32 value against it)"""
    zero = 0.0
    if isinstance(fac, str):
        return (t if fac == "t" else x[:, COORDS[fac]]), zero
    c, name = fac
    C = len(nt)
    if name in MIXED:
        k = MIXED[name]
        a, b = PAIRS[k]
        assert pair[c][k] == 2 and nx[c][a] >= 2 and nx[c][b] >= 2, (fac, pair[c], nx[c])
        (ba, ra), (bb, rb) = axis_row(c, a, nt), axis_row(c, b, nt)
        A, B, P = jets[ba][ra], jets[bb][rb], jets[3 * C + 3 * c + k][2]
        return 0.5 * ((P - A) - B), D2 * EPS * 0.5 * (np.abs(P) + np.abs(A) + np.abs(B))
    u = jets[3 * c][0]
    if name == "sin(u)":
        return np.sin(u), zero
    if name == "cos(u)":
        return np.cos(u), zero
    b, row = M2.stream_of(name, nt[c], nx[c])
    return jets[3 * c + b][row], zero


def evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, eq_weights=None, loss="mse", delta=1.0, grad_scale=1.0,
             residual_cotangent=None):
    """Everything `pinn_term_residual_system_mixed` returns, in fp64, with bounds: the keys of `term_system_model.evaluate`,
    cot / cot_bound / touched being lists of 6 C blocks."""
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
    F = max([len(f) for _, f in terms] + [0])
    T_e = [sum(1 for e, _ in terms if e == k) for k in range(E)]

    r, A, Ed = np.zeros((E, N)), np.zeros((E, N)), np.zeros((E, N))
    prod_all = np.ones((T, N))
    summands = []  # per term: list of (block, row, value, |.| on the widened factors, the same minus |.| on the exact ones)
    for m, (e, factors) in enumerate(terms):
        vals = [_value(f, dim, nt, nx, pair, jets, x, t) for f in factors]
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
                continue
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


# ---- the programs of tests/test_term_system_mixed_kernel_gpu.py ------------------------------------------------------------
def _u(c, name="u"):
    return (c, name)


def _elasticity2d(mu=0.5, a=1.3):
    """u_t = mu Lap u + a (u_xx + v_xy),  v_t = mu Lap v + a (u_xy + v_yy), a = lambda + mu: each field names the other's mixed
    derivative."""
    u, v = 0, 1
    terms = [(0, (_u(u, "u_t"),)), (0, (_u(u, "u_xx"),)), (0, (_u(u, "u_yy"),)), (0, (_u(u, "u_xx"),)), (0, (_u(v, "u_xy"),)),
             (1, (_u(v, "u_t"),)), (1, (_u(v, "u_xx"),)), (1, (_u(v, "u_yy"),)), (1, (_u(u, "u_xy"),)), (1, (_u(v, "u_yy"),))]
    coef = [1.0, -mu, -mu, -a, -a, 1.0, -mu, -mu, -a, -a]
    return 2, (1, 1), ((2, 2, 0), (2, 2, 0)), ((2, 0, 0), (2, 0, 0)), 2, terms, coef


def _elasticity3d(mu=0.5, a=1.3):
    """The same in 3-D, fields (u, v, w): all three pairs, each field naming two (u: xy, xz; v: xy, yz; w: xz, yz)."""
    u, v, w = 0, 1, 2
    terms, coef = [], []
    grad_div = {u: ((u, "u_xx"), (v, "u_xy"), (w, "u_xz")), v: ((u, "u_xy"), (v, "u_yy"), (w, "u_yz")),
                w: ((u, "u_xz"), (v, "u_yz"), (w, "u_zz"))}
    for e in (u, v, w):
        terms += [(e, (_u(e, "u_t"),))] + [(e, (_u(e, n),)) for n in ("u_xx", "u_yy", "u_zz")] + [(e, (f,)) for f in grad_div[e]]
        coef += [1.0, -mu, -mu, -mu, -a, -a, -a]
    return 3, (1, 1, 1), ((2, 2, 2),) * 3, ((2, 2, 0), (2, 0, 2), (0, 2, 2)), 3, terms, coef


def _caps():
    """The LDS maximum: C = E = 4, dimension 3, 32 terms of up to 4 factors, every field naming all three pairs; a sin, a cos
    and coordinate factors; a term with the same mixed factor twice (two summands into one g); the rest is drawn from every
    field's streams with a fixed seed."""
    nt = (2, 1, 1, 1)
    nx = ((2, 2, 2), (4, 2, 2), (2, 2, 2), (3, 2, 2))
    pair = ((2, 2, 2),) * 4
    names = []
    for c in range(4):
        have = ["u", "sin(u)", "cos(u)"] + ["u_t", "u_tt"][: nt[c]] + ["u_x", "u_xx", "u_xxx", "u_xxxx"][: nx[c][0]]
        names.append(have + ["u_y", "u_yy", "u_z", "u_zz", "u_xy", "u_xz", "u_yz"])
    fixed = [
        (0, (_u(0, "u_xy"), _u(0, "u_xy"), _u(1), "x")),                     # the same mixed factor twice: two summands, one g
        (1, (_u(0, "u_xz"), _u(1, "u_xz"), _u(2, "u_xz"), _u(3, "u_xz"))),   # one mixed factor of every field
        (2, (_u(0, "u_yz"), _u(0, "u_yy"), _u(0, "u_zz"), _u(0, "sin(u)"))), # a mixed factor beside the axis rows it is made of
        (3, (_u(1, "u_xy"), _u(1, "u_xx"), _u(1, "cos(u)"), "t")),
        (0, (_u(1, "u_yz"), _u(2, "u_xy"), "y", "z")),
        (1, (_u(2, "u_yz"), _u(3, "u_xy"), _u(3, "u_yz"))),
        (2, (_u(0), _u(0), _u(0, "sin(u)"), _u(0, "cos(u)"))),               # four summands into one accumulator
        (3, ("x", "y", "z", "t")),                                           # coordinates only: no cotangent at all
    ]
    rng = np.random.default_rng(20241)
    terms = list(fixed)
    while len(terms) < 32:
        factors = []
        for _ in range(int(rng.integers(1, 5))):
            k = int(rng.integers(0, 10))
            if k == 0:
                factors.append(["x", "y", "z", "t"][int(rng.integers(0, 4))])
            else:
                c = int(rng.integers(0, 4))
                factors.append((c, names[c][int(rng.integers(0, len(names[c])))]))
        terms.append((len(terms) % 4, tuple(factors)))
    coef = [float(v) for v in np.round(rng.uniform(0.2, 1.2, 32) * rng.choice([-1.0, 1.0], 32), 3)]
    return 3, nt, nx, pair, 4, terms, coef


def _one_pair():
    """Three fields in 3-D; only field 1 names a mixed derivative, u_xz: the P blocks of the fields 0 and 2 (and the two other
    pairs of field 1) are NULL.  No term names field 2, whose blocks must come back all zero."""
    terms = [(0, (_u(0, "u_t"),)), (0, (_u(0, "u_xx"),)), (0, (_u(0, "u_yy"),)), (0, (_u(1, "u_xz"),)),
             (1, (_u(1, "u_t"),)), (1, (_u(1, "u_xx"),)), (1, (_u(1, "u_zz"),)), (1, (_u(0), _u(1, "u_xz"))), (1, ("z", _u(1, "u_z")))]
    coef = [1.0, -0.4, -0.4, -0.9, 1.0, -0.3, -0.3, 0.6, 0.25]
    return 3, (1, 1, 1), ((2, 2, 0), (2, 0, 2), (1, 1, 0)), ((0, 0, 0), (0, 2, 0), (0, 0, 0)), 2, terms, coef


def _no_mixed():
    """`navier_stokes` of the sibling model with all pair orders 0: the pure-term rounding order is the sibling kernel's."""
    dim, nt, nx, n_eq, terms, coef = SM.PROGRAMS["navier_stokes"]
    return dim, nt, nx, ((0, 0, 0),) * len(nt), n_eq, terms, coef


PROGRAMS = {"elasticity2d": _elasticity2d(), "elasticity3d": _elasticity3d(), "caps": _caps(), "one_pair": _one_pair(),
            "no_mixed": _no_mixed()}
EQ_WEIGHTS = {"elasticity2d": (1.0, 2.0), "elasticity3d": (1.0, 0.5, 2.0), "caps": (1.0, 0.5, 0.25, 2.0), "one_pair": (1.0, 0.0),
              "no_mixed": SM.EQ_WEIGHTS["navier_stokes"]}

# (program, size) whose default seed puts more than 1 % of the points within their bound of a kink of l' (checked on the model
# alone in tests/test_term_system_mixed_cpu.py): the next seed is taken
_SEED_SHIFT = {}


def inputs(name, N, seed=None):
    """Standard-normal jets and coordinates in fp32, the program's coefficients and a standard-normal (E, N) cotangent, seeded
    per (program, size).  `no_mixed` takes the sibling's inputs of `navier_stokes`, so both kernels can run on the same data."""
    dim, nt, nx, pair, n_eq, terms, coef = PROGRAMS[name]
    if name == "no_mixed":
        _, _, _, _, _, c32, jets, x, t, rbar = SM.inputs("navier_stokes", N, seed)
        return dim, nt, nx, pair, n_eq, terms, c32, jets + [None] * (3 * len(nt)), x, t, rbar
    if seed is None:
        seed = 19000 + 1000 * sorted(PROGRAMS).index(name) + N + _SEED_SHIFT.get((name, N), 0)
    rng = np.random.default_rng(seed)
    jets = [None if s is None else rng.standard_normal(s).astype(np.float32) for s in block_shapes(dim, nt, nx, pair, N)]
    x = rng.standard_normal((N, dim)).astype(np.float32)
    t = rng.standard_normal(N).astype(np.float32)
    rbar = rng.standard_normal((n_eq, N)).astype(np.float32)
    return dim, nt, nx, pair, n_eq, terms, np.asarray(coef, dtype=np.float32), jets, x, t, rbar


def engine_terms(terms):
    """(factors per term, equation_of) in the form `engine.MixedSystemTermDesc` takes."""
    return [f for _, f in terms], [e for e, _ in terms]
