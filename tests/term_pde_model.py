"""fp64 specification of `pinn_term_residual` (include/pinn_jet.h) in numpy, with a per-point error bound.

A program is (nt, nx, terms) with terms a list of factor-name tuples; the inputs (coefficients, jets, coordinates) are the
fp32 numbers the kernel reads, widened to fp64, so the model's only error is fp64's own.

The bound.  With A_n = sum_m |c_m| prod_f |phi_{m,f}|, T terms and F = the largest factor count of a term, an fp32
evaluation of r_n rounds at most F times inside a product (relative to that product), once or twice more where a factor is
the device's sin / cos (about 1 ulp), and T - 1 times while adding the terms (relative to a partial sum, which never
exceeds A_n in magnitude): at most T + F + 2 half-ulp roundings relative to A_n, i.e. (T + F + 2) 2^-24 A_n.  The bound
used is twice that, (T + F + 2) 2^-23 A_n, to cover the order of the adds, fused multiply-adds and sin / cos.
dr/djet_s gets the same bound with its own absolute sum (one summand per factor position that names the stream, sin(u) and
cos(u) counting towards u): the kernel adds the at most four summands of one term first and the terms after that, so
the count of roundings does not grow with the program.  The cotangent rbar dr/djet_s carries that bound through l'.
"""

import numpy as np

FACTORS = ("u", "u_t", "u_tt", "u_x", "u_xx", "u_xxx", "u_xxxx", "x", "t", "sin(u)", "cos(u)")
T_ORDER = {"u_t": 1, "u_tt": 2}
X_ORDER = {"u_x": 1, "u_xx": 2, "u_xxx": 3, "u_xxxx": 4}
EPS = 2.0 ** -23


def stream_of(name, nt, nx):
    """Row of the (K, N) jets that holds the factor `name`, or None for a factor that is not a stream."""
    if name == "u":
        return 0
    if name in T_ORDER:
        assert T_ORDER[name] <= nt, (name, nt)
        return T_ORDER[name]
    if name in X_ORDER:
        assert X_ORDER[name] <= nx, (name, nx)
        return nt + X_ORDER[name]
    return None


def _values(nt, nx, jets, x, t):
    u = jets[0]
    v = {"u": u, "x": x, "t": t, "sin(u)": np.sin(u), "cos(u)": np.cos(u)}
    for name, k in T_ORDER.items():
        if k <= nt:
            v[name] = jets[k]
    for name, k in X_ORDER.items():
        if k <= nx:
            v[name] = jets[nt + k]
    return v


def loss_and_slope(r, loss, delta):
    """l(r), l'(r) per sample as PDEBase._apply_loss_fn has them before the mean: sgn(0) = 0, Huber quadratic on |r| < delta."""
    if loss == "mae":
        return np.abs(r), np.sign(r)
    if loss == "huber":
        a = np.abs(r)
        quad = a < delta
        return np.where(quad, 0.5 * r * r, delta * (a - 0.5 * delta)), np.where(quad, r, delta * np.sign(r))
    return r * r, 2.0 * r


def evaluate(nt, nx, terms, coef, jets, x, t, loss="mse", delta=1.0, grad_scale=1.0, residual_cotangent=None):
    """Everything `pinn_term_residual` returns, in fp64, with bounds.  jets: (K, N); coef: (T,); x, t: (N,).

    r, r_bound                    residual and its fp32 error bound per point
    dr, dr_bound                  (K, N): dr/djet_s and its bound
    loss_sum, loss_abs            sum_n l(r_n) and sum_n |l(r_n)|
    rbar, rbar_bound              grad_scale l'(r_n) (or the given cotangent) and what r_bound does to it
    cot, cot_bound                (K, N): rbar dr/djet_s
    coef_sums, coef_abs           (T,): sum_n rbar_n prod_f phi and the sum of the absolute summands
    coef_prod                     (T, N): prod_f phi_{m,f}
    unsafe                        (N,) bool: |r| within its bound of the kink of l' (0 for mae, delta for huber), where the
                                  device may take the other branch
    """
    K, N = 1 + nt + nx, jets.shape[1]
    assert jets.shape == (K, N)
    coef = np.asarray(coef, dtype=np.float64)
    jets = np.asarray(jets, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    v = _values(nt, nx, jets, x, t)
    T = len(terms)
    F = max([len(f) for f in terms] + [0])
    r, A = np.zeros(N), np.zeros(N)
    dr, dA = np.zeros((K, N)), np.zeros((K, N))
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
            if name in ("x", "t"):
                continue
            others = coef[m] * np.ones(N)
            for g, ph in enumerate(phi):
                if g != f:
                    others = others * ph
            if name == "sin(u)":
                s, term = 0, others * v["cos(u)"]
            elif name == "cos(u)":
                s, term = 0, -others * v["sin(u)"]
            else:
                s, term = stream_of(name, nt, nx), others
            dr[s] += term
            dA[s] += np.abs(term)
    count = T + F + 2
    r_bound, dr_bound = count * EPS * A, count * EPS * dA
    lv, slope = loss_and_slope(r, loss, delta)
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
    cot = rbar[None, :] * dr
    # rbar's own bound, dr's bound, and the two fp32 roundings of grad_scale * l' and rbar * dr (twice the half ulp each)
    cot_bound = np.abs(rbar)[None, :] * dr_bound + rbar_bound[None, :] * (np.abs(dr) + dr_bound) + 2 * EPS * np.abs(cot)
    summands = rbar[None, :] * prod_all
    return {"r": r, "r_bound": r_bound, "dr": dr, "dr_bound": dr_bound, "loss_sum": lv.sum(), "loss_abs": np.abs(lv).sum(),
            "rbar": rbar, "rbar_bound": rbar_bound, "cot": cot, "cot_bound": cot_bound, "coef_sums": summands.sum(1),
            "coef_abs": np.abs(summands).sum(1), "coef_prod": prod_all, "unsafe": unsafe, "count": count}


# ---- the programs of tests/test_term_kernel_gpu.py (stream set, terms, O(1) coefficients) --------------------------------
PROGRAMS = {
    "burgers": (1, 2, [("u_t",), ("u", "u_x"), ("u_xx",)], [1.0, 1.0, -0.05]),
    "kuramoto_sivashinsky": (1, 4, [("u_t",), ("u", "u_x"), ("u_xx",), ("u_xxxx",)], [1.0, 1.0, 1.0, 1.0]),
    "cubic_klein_gordon": (2, 2, [("u_tt",), ("u_xx",), ("u", "u", "u")], [1.0, -1.0, 1.0]),
    "pendulum": (2, 0, [("u_tt",), ("sin(u)",)], [1.0, 9.81]),
    "black_scholes": (1, 2, [("u_t",), ("x", "x", "u_xx"), ("x", "u_x"), ("u",)], [1.0, 0.02, 0.05, -0.05]),
    "sixteen": (1, 4, [(), ("t",), ("u",), ("u_t",), ("u_x",), ("u_xx",), ("u_xxx",), ("u_xxxx",), ("u", "u"), ("u", "u_x"),
                       ("x", "u_xx"), ("t", "u", "u_x"), ("sin(u)", "u_x"), ("cos(u)", "u_t"), ("u", "u", "u", "u"),
                       ("x", "t", "cos(u)", "sin(u)")],
                [0.3, -0.7, 1.1, 1.0, -0.6, 0.8, 0.25, -0.4, 0.5, 1.3, -0.9, 0.45, 0.75, -1.2, 0.15, 0.65]),
}
SIZES = (1, 37, 1027, 16421)
LOSSES = (("mse", 1.0), ("mae", 1.0), ("huber", 0.75))


# (program, size) whose default seed puts a point within its bound of a kink of l' (tests/test_term_pde_cpu.py checks that
# none is left): the next seed is taken
_SEED_SHIFT = {("sixteen", 16421): 1}


def inputs(name, N, seed=None):
    """Standard-normal jets and coordinates in fp32 and the program's coefficients, seeded per (program, size)."""
    nt, nx, terms, coef = PROGRAMS[name]
    if seed is None:
        seed = 1000 * sorted(PROGRAMS).index(name) + N + _SEED_SHIFT.get((name, N), 0)
    rng = np.random.default_rng(seed)
    K = 1 + nt + nx
    jets = rng.standard_normal((K, N)).astype(np.float32)
    x = rng.standard_normal(N).astype(np.float32)
    t = rng.standard_normal(N).astype(np.float32)
    rbar = rng.standard_normal(N).astype(np.float32)
    return nt, nx, terms, np.asarray(coef, dtype=np.float32), jets, x, t, rbar
