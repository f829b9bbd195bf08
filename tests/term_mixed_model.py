"""fp64 specification of `pinn_term_residual_mixed` (include/pinn_jet.h) in numpy, with a per-point error bound.

A program is (dimension, nt, (nx0, nx1, nx2), (pair_xy, pair_xz, pair_yz), terms).  The inputs are the fp32 numbers the
kernel reads, widened to fp64: the coefficients, the 9 blocks [axis0, axis1, axis2, P_xy, P_xz, P_yz, Q_xy, Q_xz, Q_yz] (axis
blocks as in tests/term_nd_model.py with up to four space rows; P_ab the (1 + pair order, N) block of the launch along
e_a + e_b, Q_ab the (5, N) block along e_a - e_b of a pair of order 4; None where the program has no such block), x and t.

The derived factors are the header's formulas,
    u_ab   = 0.5 ((P_2 - A_2) - B_2),        u_aabb = ((P_4 + Q_4) - 2 (A_4 + B_4)) / 12,
with A_k, B_k the order-k rows of the two axis blocks.

The bound extends the argument of tests/term_nd_model.py by the roundings of the two formulas in their stated order.
u_ab takes two fp32 roundings (the two subtractions; the product with 0.5 is exact), each at most 2^-24 of a partial result
no larger than |P_2| + |A_2| + |B_2|: the fp32 value is within D2 EPS S_2 of the fp64 one, D2 = 2, S_2 = (|P_2| + |A_2| +
|B_2|) / 2, EPS = 2^-23 (twice the unit roundoff, as everywhere in these models).  u_aabb takes five (two sums, the
subtraction — the product with 2 is exact —, the product with the constant and the constant (float)(1 / 12) itself): within
D4 EPS S_4, D4 = 5, S_4 = (|P_4| + |Q_4| + 2 |A_4| + 2 |B_4|) / 12.  A factor that is off by d enters a product of the
term loop as |phi| + d at most, so the residual and dr/dfactor are within
    (T + F + 2) EPS  sum_m |c_m| prod_f (|phi| + d)   +   sum_m |c_m| (prod_f (|phi| + d) - prod_f |phi|)
of the fp64 ones: tests/term_nd_model.py's bound on the widened absolute sum, plus what the factor errors move.  With no
derived factor d = 0 everywhere and both expressions are term_nd_model's, bit for bit.
The transposed maps run once per point: g/2 is exact, h (float)(1 / 12) takes two roundings, and every subtraction from an
axis row one more, of the row's new value.
"""

import numpy as np

import term_nd_model as ND
import term_pde_model as M1

FACTORS = ND.FACTORS + ("u_yyy", "u_yyyy", "u_zzz", "u_zzzz", "u_xy", "u_xz", "u_yz", "u_xxyy", "u_xxzz", "u_yyzz")
CODES = {name: i for i, name in enumerate(FACTORS)}
AXIS_ORDER = dict(ND.AXIS_ORDER, u_yyy=(1, 3), u_yyyy=(1, 4), u_zzz=(2, 3), u_zzzz=(2, 4))
PAIRS = ((0, 1), (0, 2), (1, 2))
MIXED = {"u_xy": (0, 2), "u_xz": (1, 2), "u_yz": (2, 2), "u_xxyy": (0, 4), "u_xxzz": (1, 4), "u_yyzz": (2, 4)}  # (pair, order)
COORDS = ND.COORDS
EPS = M1.EPS
D2, D4 = 2, 5
BLOCKS = 9


def axis_row(a, k, nt):
    """(block, row) of the order-k derivative along axis a."""
    return (0, nt + k) if a == 0 else (a, k)


def block_rows(dim, nt, nx, pair):
    rows = [1 + nt + nx[0]] + [(1 + nx[a]) if (a < dim and nx[a] > 0) else 0 for a in (1, 2)]
    return rows + [(1 + pair[k]) if pair[k] >= 2 else 0 for k in range(3)] + [5 if pair[k] == 4 else 0 for k in range(3)]


def stream_of(name, nt, nx):
    if name in AXIS_ORDER:
        a, k = AXIS_ORDER[name]
        assert k <= nx[a], (name, nx)
        return a, k
    row = M1.stream_of(name, nt, nx[0])
    return None if row is None else (0, row)


def _values(dim, nt, nx, pair, jets, x, t):
    """factor name -> (value, absolute error of the fp32 value against it)"""
    N = jets[0].shape[1]
    zero = np.zeros(N)
    u = jets[0][0]
    v = {"u": u, "t": t, "sin(u)": np.sin(u), "cos(u)": np.cos(u)}
    for name, a in COORDS.items():
        if a < dim:
            v[name] = x[:, a]
    for name, k in M1.T_ORDER.items():
        if k <= nt:
            v[name] = jets[0][k]
    for name, k in M1.X_ORDER.items():
        if k <= nx[0]:
            v[name] = jets[0][nt + k]
    for name, (a, k) in AXIS_ORDER.items():
        if a < dim and k <= nx[a]:
            v[name] = jets[a][k]
    dv = {name: zero for name in v}
    for name, (k, o) in MIXED.items():
        a, b = PAIRS[k]
        if pair[k] < o or nx[a] < o or nx[b] < o or (o == 4 and (nx[a] != 4 or nx[b] != 4)):
            continue
        (ba, ra), (bb, rb) = axis_row(a, o, nt), axis_row(b, o, nt)
        A, B, P = jets[ba][ra], jets[bb][rb], jets[3 + k][o]
        if o == 2:
            v[name] = 0.5 * ((P - A) - B)
            dv[name] = D2 * EPS * 0.5 * (np.abs(P) + np.abs(A) + np.abs(B))
        else:
            Q = jets[6 + k][4]
            v[name] = ((P + Q) - 2.0 * (A + B)) / 12.0
            dv[name] = D4 * EPS * (np.abs(P) + np.abs(Q) + 2.0 * np.abs(A) + 2.0 * np.abs(B)) / 12.0
    return v, dv


def evaluate(dim, nt, nx, pair, terms, coef, jets, x, t, loss="mse", delta=1.0, grad_scale=1.0, residual_cotangent=None):
    """Everything `pinn_term_residual_mixed` returns, in fp64, with bounds.  The keys are those of
    `term_nd_model.evaluate`; dr, dr_bound, cot and cot_bound are lists of 9 blocks (None where the program has no such
    block).  Every row the program never reads is zero with a zero bound."""
    N = jets[0].shape[1]
    nx = tuple(nx) + (0,) * (3 - len(nx))
    pair = tuple(pair) + (0,) * (3 - len(pair))
    coef = np.asarray(coef, dtype=np.float64)
    jets = [None if j is None else np.asarray(j, dtype=np.float64) for j in jets] + [None] * (BLOCKS - len(jets))
    rows = block_rows(dim, nt, nx, pair)
    for b in range(BLOCKS):
        assert (jets[b] is None) == (rows[b] == 0) and (jets[b] is None or jets[b].shape == (rows[b], N)), (b, rows)
    x = np.asarray(x, dtype=np.float64).reshape(N, dim)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    v, dv = _values(dim, nt, nx, pair, jets, x, t)
    T = len(terms)
    F = max([len(f) for f in terms] + [0])
    r, A, E = np.zeros(N), np.zeros(N), np.zeros(N)
    G, GA, GE = {}, {}, {}  # per factor name: dr/dfactor, its absolute sum (widened), what the factor errors move

    def slot(name):
        if name not in G:
            G[name], GA[name], GE[name] = np.zeros(N), np.zeros(N), np.zeros(N)
        return name

    prod_all = np.ones((T, N))
    for m, factors in enumerate(terms):
        phi = [v[f] for f in factors]
        wide = [np.abs(v[f]) + dv[f] for f in factors]
        p, pa, pw = np.ones(N), np.ones(N), np.ones(N)
        for ph, w in zip(phi, wide):
            p = p * ph
            pa = pa * np.abs(ph)
            pw = pw * w
        prod_all[m] = p
        r += coef[m] * p
        A += abs(coef[m]) * pw
        E += abs(coef[m]) * (pw - pa)
        for f, name in enumerate(factors):
            if name in COORDS or name == "t":
                continue
            others, oa, ow = coef[m] * np.ones(N), abs(coef[m]) * np.ones(N), abs(coef[m]) * np.ones(N)
            for g, (ph, w) in enumerate(zip(phi, wide)):
                if g != f:
                    others = others * ph
                    oa = oa * np.abs(ph)
                    ow = ow * w
            if name == "sin(u)":
                key, term, scale = slot("u"), others * v["cos(u)"], np.abs(v["cos(u)"])
            elif name == "cos(u)":
                key, term, scale = slot("u"), -others * v["sin(u)"], np.abs(v["sin(u)"])
            else:
                key, term, scale = slot(name), others, 1.0
            G[key] += term
            GA[key] += ow * scale
            GE[key] += (ow - oa) * scale
    count = T + F + 2
    r_bound = count * EPS * A + E
    dr = [None if k == 0 else np.zeros((k, N)) for k in rows]
    db = [None if k == 0 else np.zeros((k, N)) for k in rows]
    for name in G:
        if name in MIXED:
            continue
        b, s = stream_of(name, nt, nx)
        dr[b][s] += G[name]
        db[b][s] += count * EPS * GA[name] + GE[name]
    for name in G:  # the transposed maps
        if name not in MIXED:
            continue
        k, o = MIXED[name]
        g, gb = G[name], count * EPS * GA[name] + GE[name]
        if o == 2:
            share, share_b, blocks = 0.5 * g, 0.5 * gb, (3 + k,)
        else:
            share, share_b, blocks = g / 12.0, gb / 12.0 + 2 * EPS * np.abs(g) / 12.0, (3 + k, 6 + k)
        for b in blocks:
            dr[b][o] += share
            db[b][o] += share_b
        for a in PAIRS[k]:
            b, s = axis_row(a, o, nt)
            w = 1.0 if o == 2 else 2.0
            dr[b][s] -= w * share
            db[b][s] += w * share_b
            db[b][s] += EPS * (np.abs(dr[b][s]) + db[b][s])
    lv, slope = M1.loss_and_slope(r, loss, delta)
    if residual_cotangent is not None:
        rbar = np.asarray(residual_cotangent, dtype=np.float64).reshape(-1)
        rbar_bound = np.zeros(N)
        unsafe = np.zeros(N, dtype=bool)
    else:
        rbar = grad_scale * slope
        if loss == "mae":
            rbar_bound = np.zeros(N)
            unsafe = np.abs(r) <= r_bound
        elif loss == "huber":
            rbar_bound = np.where(np.abs(r) < delta, abs(grad_scale) * r_bound, 0.0)
            unsafe = np.abs(np.abs(r) - delta) <= r_bound
        else:
            rbar_bound = 2.0 * abs(grad_scale) * r_bound
            unsafe = np.zeros(N, dtype=bool)
    cot = [None if d is None else rbar[None, :] * d for d in dr]
    cot_bound = [None if d is None else
                 np.abs(rbar)[None, :] * b_ + rbar_bound[None, :] * (np.abs(d) + b_) + 2 * EPS * np.abs(c)
                 for d, b_, c in zip(dr, db, cot)]
    summands = rbar[None, :] * prod_all
    # the coefficient sums multiply fp32 factor values: what the factor errors move in them, summed over the points
    coef_in = np.zeros(T)
    for m, factors in enumerate(terms):
        pa, pw = np.ones(N), np.ones(N)
        for f in factors:
            pa = pa * np.abs(v[f])
            pw = pw * (np.abs(v[f]) + dv[f])
        coef_in[m] = float((np.abs(rbar) * (pw - pa)).sum())
    return {"r": r, "r_bound": r_bound, "dr": dr, "dr_bound": db, "loss_sum": lv.sum(), "loss_abs": np.abs(lv).sum(),
            "rbar": rbar, "rbar_bound": rbar_bound, "cot": cot, "cot_bound": cot_bound, "coef_sums": summands.sum(1),
            "coef_abs": np.abs(summands).sum(1), "coef_prod": prod_all, "coef_in": coef_in, "unsafe": unsafe, "count": count}


# ---- the programs of tests/test_term_mixed_kernel_gpu.py: (dimension, nt, nx, pair, terms, O(1) coefficients) ---------------
PROGRAMS = {
    "uxy": (2, 1, (2, 2, 0), (2, 0, 0), [("u_xy",)], [1.0]),
    "monge_ampere": (2, 1, (2, 2, 0), (2, 0, 0), [("u_xx", "u_yy"), ("u_xy", "u_xy")], [1.0, -1.0]),
    "bilaplacian2d": (2, 1, (4, 4, 0), (4, 0, 0), [("u_t",), ("u_xxxx",), ("u_xxyy",), ("u_yyyy",)], [1.0, 0.1, 0.2, 0.1]),
    # all three pairs, of both orders, beside orders 3 and 4 along z
    "pairs3d": (3, 1, (4, 2, 4), (2, 4, 2), [("u_t",), ("u_xy",), ("u_xz",), ("u_yz",), ("u_xxzz",), ("u_zzz",), ("u_zzzz", "u")],
                [1.0, 0.5, -0.7, 0.9, 0.3, -0.4, 0.6]),
    # a pair that does not touch axis 0, at order 4: axis 0 carries the value and the time stream alone
    "bilaplacian_yz": (3, 1, (0, 4, 4), (0, 0, 4), [("u_t",), ("u_yyyy",), ("u_yyzz",), ("u_zzzz",), ("z", "u_yz")],
                       [1.0, 0.1, 0.2, 0.1, -0.3]),
    # sin(u), coordinate factors and a repeated derived factor: the coefficient sums see every kind of factor
    "trig_coord": (2, 1, (4, 4, 0), (4, 0, 0), [("u_t",), ("sin(u)", "u_xy"), ("y", "u_yyy"), ("x", "u_xxyy", "u_xy"), ("cos(u)",),
                                               ("u_xy", "u_xy", "u")],
                   [1.0, 0.8, -0.6, 0.4, 0.3, -0.5]),
}
SIZES = (1, 255, 257, 64 * 256 + 1)
LOSSES = M1.LOSSES
_SEED_SHIFT = {}


def inputs(name, N, seed=None):
    """Standard-normal blocks and coordinates in fp32 and the program's coefficients, seeded per (program, size)."""
    dim, nt, nx, pair, terms, coef = PROGRAMS[name]
    if seed is None:
        seed = 7000 + 1000 * sorted(PROGRAMS).index(name) + N + _SEED_SHIFT.get((name, N), 0)
    rng = np.random.default_rng(seed)
    jets = [rng.standard_normal((k, N)).astype(np.float32) if k else None for k in block_rows(dim, nt, nx, pair)]
    x = rng.standard_normal((N, dim)).astype(np.float32)
    t = rng.standard_normal(N).astype(np.float32)
    rbar = rng.standard_normal(N).astype(np.float32)
    return dim, nt, nx, pair, terms, np.asarray(coef, dtype=np.float32), jets, x, t, rbar
