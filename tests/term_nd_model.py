"""fp64 specification of `pinn_term_residual_axes` (include/pinn_jet.h) in numpy, with a per-point error bound.

A program is (dimension, nt, (nx0, nx1, nx2), terms) with terms a list of factor-name tuples.  The inputs are the fp32
numbers the kernel reads, widened to fp64: the coefficients, one block of jets per axis (block 0: (1 + nt + nx0, N) in the
order [u, d/dt.., d/dx..]; block a >= 1: (1 + nx_a, N) = [u, d/dx_a, d2/dx_a2], None when nx_a = 0; row 0 of a block >= 1 is
the value stream again and is never read), x (N, dimension) and t (N,).

The bound is the one of tests/term_pde_model.py, whose argument does not depend on where a factor comes from: with
A_n = sum_m |c_m| prod_f |phi_{m,f}|, T terms and F the largest factor count, the fp32 residual is within
(T + F + 2) 2^-23 A_n of the fp64 one, and dr/d(stream) within the same multiple of its own absolute sum (the kernel sums the
at most four summands of one term first, then the terms).  The cotangent rbar dr/d(stream) carries that bound through l'.
"""

import numpy as np

import term_pde_model as M1

FACTORS = M1.FACTORS + ("u_y", "u_yy", "u_z", "u_zz", "y", "z")
CODES = {name: i for i, name in enumerate(FACTORS)}
AXIS_ORDER = {"u_y": (1, 1), "u_yy": (1, 2), "u_z": (2, 1), "u_zz": (2, 2)}  # factor -> (axis, order)
COORDS = {"x": 0, "y": 1, "z": 2}
EPS = M1.EPS


def stream_of(name, nt, nx):
    """(block, row) of the factor `name`, or None for a factor that is not a stream.  nx = (nx0, nx1, nx2)."""
    if name in AXIS_ORDER:
        a, k = AXIS_ORDER[name]
        assert k <= nx[a], (name, nx)
        return a, k
    row = M1.stream_of(name, nt, nx[0])
    return None if row is None else (0, row)


def _values(dim, nt, nx, jets, x, t):
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
    return v


def evaluate(dim, nt, nx, terms, coef, jets, x, t, loss="mse", delta=1.0, grad_scale=1.0, residual_cotangent=None):
    """Everything `pinn_term_residual_axes` returns, in fp64, with bounds.  The keys are those of
    `term_pde_model.evaluate`; dr, dr_bound, cot and cot_bound are LISTS with one (rows, N) array per block (None where the
    axis has no streams), and row 0 of every block >= 1 is zero with a zero bound: the whole cotangent of u, sin(u) and cos(u)
    belongs to row 0 of block 0."""
    N = jets[0].shape[1]
    nx = tuple(nx) + (0,) * (3 - len(nx))
    coef = np.asarray(coef, dtype=np.float64)
    jets = [None if j is None else np.asarray(j, dtype=np.float64) for j in jets] + [None] * (3 - len(jets))
    assert jets[0].shape == (1 + nt + nx[0], N)
    for a in (1, 2):
        assert (jets[a] is None) == (a >= dim or nx[a] == 0), (a, dim, nx)
    x = np.asarray(x, dtype=np.float64).reshape(N, dim)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    v = _values(dim, nt, nx, jets, x, t)
    T = len(terms)
    F = max([len(f) for f in terms] + [0])
    r, A = np.zeros(N), np.zeros(N)
    shapes = [(1 + nt + nx[0], N)] + [(1 + nx[a], N) if (a < dim and nx[a] > 0) else None for a in (1, 2)]
    dr = [None if s is None else np.zeros(s) for s in shapes]
    dA = [None if s is None else np.zeros(s) for s in shapes]
    prod_all = np.ones((T, N))
    for m, factors in enumerate(terms):
        phi = [v[f] for f in factors]
        p = np.ones(N)
        for ph in phi:
            p = p * ph
        prod_all[m] = p
        r += coef[m] * p
        A += abs(coef[m]) * np.abs(p)
        for f, name in enumerate(factors):
            if name in COORDS or name == "t":
                continue
            others = coef[m] * np.ones(N)
            for g, ph in enumerate(phi):
                if g != f:
                    others = others * ph
            if name == "sin(u)":
                (b, s), term = (0, 0), others * v["cos(u)"]
            elif name == "cos(u)":
                (b, s), term = (0, 0), -others * v["sin(u)"]
            else:
                (b, s), term = stream_of(name, nt, nx), others
            dr[b][s] += term
            dA[b][s] += np.abs(term)
    count = T + F + 2
    r_bound = count * EPS * A
    dr_bound = [None if a is None else count * EPS * a for a in dA]
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
    # rbar's own bound, dr's bound, and the two fp32 roundings of grad_scale * l' and rbar * dr (twice the half ulp each)
    cot_bound = [None if d is None else
                 np.abs(rbar)[None, :] * db + rbar_bound[None, :] * (np.abs(d) + db) + 2 * EPS * np.abs(c)
                 for d, db, c in zip(dr, dr_bound, cot)]
    summands = rbar[None, :] * prod_all
    return {"r": r, "r_bound": r_bound, "dr": dr, "dr_bound": dr_bound, "loss_sum": lv.sum(), "loss_abs": np.abs(lv).sum(),
            "rbar": rbar, "rbar_bound": rbar_bound, "cot": cot, "cot_bound": cot_bound, "coef_sums": summands.sum(1),
            "coef_abs": np.abs(summands).sum(1), "coef_prod": prod_all, "unsafe": unsafe, "count": count}


# ---- the programs of tests/test_term_nd_kernel_gpu.py: (dimension, nt, (nx0, nx1, nx2), terms, O(1) coefficients) ----------
PROGRAMS = {
    "heat2d": (2, 1, (2, 2, 0), [("u_t",), ("u_xx",), ("u_yy",)], [1.0, -0.1, -0.1]),
    "burgers2d": (2, 1, (2, 2, 0), [("u_t",), ("u", "u_x"), ("u", "u_y"), ("u_xx",), ("u_yy",)], [1.0, 1.0, 1.0, -0.05, -0.05]),
    "heat3d": (3, 1, (2, 2, 2), [("u_t",), ("u_xx",), ("u_yy",), ("u_zz",)], [1.0, -0.1, -0.1, -0.1]),
    "wave_y_only": (2, 2, (0, 2, 0), [("u_tt",), ("u_yy",), ("sin(u)",)], [1.0, -1.0, 0.5]),
    "first_order3d": (3, 1, (1, 1, 1), [("u_t",), ("x", "u_x"), ("y", "u_y"), ("z", "u_z")], [1.0, 0.5, -0.5, 0.25]),
    # every factor code, sixteen terms, up to four factors
    "every_code": (3, 2, (2, 2, 2), [(), ("t",), ("u",), ("u_t",), ("u_tt",), ("u_x",), ("u_xx",), ("u_y",), ("u_yy",), ("u_z",),
                                      ("u_zz",), ("x", "y", "z", "u"), ("sin(u)", "u_y"), ("cos(u)", "u_z", "u_zz"),
                                      ("u", "u_x", "u_y", "u_z"), ("y", "u_yy", "u_yy")],
                   [0.3, -0.7, 1.1, 1.0, -0.6, 0.8, 0.25, -0.4, 0.5, 1.3, -0.9, 0.45, 0.75, -1.2, 0.15, 0.65]),
    # the axis-0 block on its widest set, with the two x-only codes the others leave out
    "fourth_order_x": (2, 1, (4, 1, 0), [("u_t",), ("u_xxx",), ("u_xxxx",), ("u", "u_y")], [1.0, 0.5, 0.25, 1.0]),
}
SIZES = (1, 255, 257, 64 * 256 + 3)
LOSSES = M1.LOSSES

# (program, size) whose default seed puts a point within its bound of a kink of l' (tests/test_term_nd_cpu.py checks that none
# is left): the next seed is taken
_SEED_SHIFT = {}


def inputs(name, N, seed=None):
    """Standard-normal jets and coordinates in fp32 and the program's coefficients, seeded per (program, size)."""
    dim, nt, nx, terms, coef = PROGRAMS[name]
    if seed is None:
        seed = 5000 + 1000 * sorted(PROGRAMS).index(name) + N + _SEED_SHIFT.get((name, N), 0)
    rng = np.random.default_rng(seed)
    jets = [rng.standard_normal((1 + nt + nx[0], N)).astype(np.float32)]
    for a in (1, 2):
        jets.append(rng.standard_normal((1 + nx[a], N)).astype(np.float32) if (a < dim and nx[a] > 0) else None)
    x = rng.standard_normal((N, dim)).astype(np.float32)
    t = rng.standard_normal(N).astype(np.float32)
    rbar = rng.standard_normal(N).astype(np.float32)
    return dim, nt, nx, terms, np.asarray(coef, dtype=np.float32), jets, x, t, rbar
