"""fp64 numpy specification of `pinn_face_losses` (include/pinn_jet.h, "face loss terms"): term losses, every cotangent, the
summary — and the error bounds that follow from the fp32 evaluation order the header states.

Term k names up to four segments of n floats of one jets buffer (offsets in floats, None: absent):

    d_i = alpha (A[i] - A'[i]) + beta (B[i] - B'[i]) - T_i,     term_losses[k] = (1/n) sum_i l(d_i),
    cotangent: (weight / n) alpha l'(d_i) on A, its negation on A', (weight / n) beta l'(d_i) on B, its negation on B'.

The kernel's order, every operation rounded once to fp32 (u = 2^-24):
    a = A - A'  (exact without a partner);  d1 = fma(alpha, a, -T);  b = B - B';  d = fma(beta, b, d1)
so  |d_fp32 - d| <= u (|alpha a| + |alpha a - T| + |beta b| + |d|)  to first order; the model carries this bound per point
(widened by 2^-20 for the second-order terms, plus the smallest normal for underflow).

    l(d) is then taken in double from d_fp32 and summed in double: the loss of a term is off by at most the mean of
Lip_i * bound_i (Lip = |l'| on [d - bound, d + bound]) plus one rounding of the mean.
    l' is monotone for all three losses, so l'(d_fp32) lies between l'(d - bound) and l'(d + bound); the factor
fl(fl(fl(weight / n) * alpha) * l') carries three roundings: each cotangent lies in an interval the model returns.  This also
covers the kinks (|d| = 0 of mae, |d| = delta of huber), where a bound on |cot - model| would not hold.
"""

import numpy as np

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)


def loss_fn(kind, delta, d):
    if kind == "mae":
        return np.abs(d)
    if kind == "huber":
        return np.where(np.abs(d) < delta, 0.5 * d * d, delta * (np.abs(d) - 0.5 * delta))
    return d * d


def dloss_fn(kind, delta, d):
    if kind == "mae":
        return np.sign(d)
    if kind == "huber":
        return np.clip(d, -delta, delta)
    return 2.0 * d


def _lipschitz(kind, delta, d, bound):
    top = np.abs(d) + bound
    if kind == "mae":
        return np.ones_like(d)
    if kind == "huber":
        return np.minimum(top, delta)
    return 2.0 * top


def term_d(jets, tm):
    """(d, bound) of one term in fp64 from the fp32 jets."""
    J = np.asarray(jets, dtype=np.float64)
    n = int(tm["n"])
    alpha, beta = float(np.float32(tm.get("alpha", 0.0))), float(np.float32(tm.get("beta", 0.0)))
    tg = tm.get("target", 0.0)
    T = np.asarray(tg, dtype=np.float64).reshape(-1) if isinstance(tg, np.ndarray) else np.full(n, float(np.float32(tg)))
    seg = lambda name: J[tm[name] : tm[name] + n] if tm.get(name) is not None else None  # noqa: E731
    a = np.zeros(n) if seg("value") is None else seg("value") - (0.0 if seg("value_pair") is None else seg("value_pair"))
    b = np.zeros(n) if seg("deriv") is None else seg("deriv") - (0.0 if seg("deriv_pair") is None else seg("deriv_pair"))
    d1 = alpha * a - T
    d = d1 + beta * b
    bound = U * (np.abs(alpha * a) + np.abs(d1) + np.abs(beta * b) + np.abs(d)) * (1.0 + 2.0 ** -20) + TINY
    return d, bound


def face_losses_model(jets, terms, loss, delta):
    """term_losses (fp64), term_bounds, and per float of the buffer cot_lo <= cotangent <= cot_hi with `named` the mask of the
    floats some term names (every other float must be left untouched)."""
    n_floats = len(jets)
    losses, bounds = np.zeros(len(terms)), np.zeros(len(terms))
    lo, hi = np.full(n_floats, np.nan), np.full(n_floats, np.nan)
    named = np.zeros(n_floats, dtype=bool)
    for k, tm in enumerate(terms):
        n = int(tm["n"])
        d, bd = term_d(jets, tm)
        losses[k] = loss_fn(loss, delta, d).mean()
        bounds[k] = (_lipschitz(loss, delta, d, bd) * bd).mean() + 2.0 * U * abs(losses[k]) + TINY
        g0, g1 = dloss_fn(loss, delta, d - bd), dloss_fn(loss, delta, d + bd)
        s = float(np.float32(tm["weight"])) / n
        for name, pair, coef in (("value", "value_pair", tm.get("alpha", 0.0)), ("deriv", "deriv_pair", tm.get("beta", 0.0))):
            if tm.get(name) is None:
                continue
            for off, sign in ((tm[name], 1.0), (tm.get(pair), -1.0)):
                if off is None:
                    continue
                c = sign * s * float(np.float32(coef))
                e0, e1 = np.minimum(c * g0, c * g1), np.maximum(c * g0, c * g1)
                assert not named[off : off + n].any(), "the model's terms overlap"
                lo[off : off + n] = e0 - 4.0 * U * np.abs(e0) - TINY
                hi[off : off + n] = e1 + 4.0 * U * np.abs(e1) + TINY
                named[off : off + n] = True
    return {"term_losses": losses, "term_bounds": bounds, "cot_lo": lo, "cot_hi": hi, "named": named}


def summary_model(term_losses_f32, weights, residual_sum, residual_scale, residual_weight, n_boundary_terms):
    """{residual, boundary, initial, total} exactly as the finish pass forms them from the ROUNDED term losses: the residual one
    fp32 product; the three sums in double in term order, each rounded once."""
    L = np.asarray(term_losses_f32, dtype=np.float32).astype(np.float64)
    res = np.float32(0.0) if residual_sum is None else np.float32(np.float32(residual_sum) * np.float32(residual_scale))
    bnd = ini = 0.0
    tot = float(np.float32(residual_weight)) * float(res)
    for k, l in enumerate(L):
        if k < n_boundary_terms:
            bnd += l
        else:
            ini += l
        tot += float(np.float32(weights[k])) * l
    return np.array([res, np.float32(bnd), np.float32(ini), np.float32(tot)], dtype=np.float32)
