"""Executable specification of the causal (time-weighted) residual loss (include/pinn_jet.h, "causal residual weights").

Inputs are what the kernel sees: fp32 residuals, fp32 times, an fp32 sharpness.  The time bin of a point is the kernel's fp32
formula, spelt in numpy float32 (one rounded operation each); everything after it is float64, with the weights rounded to
float32 once, as the kernel stores them.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

LOSSES = ("mse", "mae", "huber")


def bins(t, n_bins: int, t_lo: float, t_hi: float) -> np.ndarray:
    """b(n) = (int) min(max((t - (float)t_lo) * s, 0), M - 1), s = (float)(M / (t_hi - t_lo)) with the quotient in double."""
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    lo = np.float32(t_lo)
    s = np.float32(np.float64(n_bins) / (np.float64(t_hi) - np.float64(t_lo)))
    v = (t - lo).astype(np.float32) * s
    v = np.minimum(np.maximum(v.astype(np.float32), np.float32(0.0)), np.float32(n_bins - 1))
    return v.astype(np.int32)


def loss_value(r: np.ndarray, loss: str, delta: float) -> np.ndarray:
    """l(r) in float64 (jet_device.h::loss_term: Huber's quadratic branch on |r| < delta)."""
    r = np.asarray(r, dtype=np.float64)
    if loss == "mae":
        return np.abs(r)
    if loss == "huber":
        d = np.float64(np.float32(delta))
        a = np.abs(r)
        return np.where(a < d, 0.5 * r * r, d * (a - 0.5 * d))
    return r * r


def loss_derivative(r: np.ndarray, loss: str, delta: float) -> np.ndarray:
    """l'(r) in float64, sgn(0) = 0."""
    r = np.asarray(r, dtype=np.float64)
    if loss == "mae":
        return np.sign(r)
    if loss == "huber":
        d = np.float64(np.float32(delta))
        return np.where(np.abs(r) < d, r, d * np.sign(r))
    return 2.0 * r


def causal_model(r, t, eps, n_bins: int, t_lo: float, t_hi: float, loss: str = "mse", delta: float = 1.0,
                 grad_scale: float = 1.0) -> SimpleNamespace:
    """bins, S, c, L, w (float32 values held in float64), L_total = (1/N) sum_n w l(r_n), plain_total = (1/N) sum_n l(r_n),
    weighted_sum / plain_sum (the unnormalised sums the kernel adds into its outputs) and rbar = grad_scale w_b(n) l'(r_n)."""
    r32 = np.asarray(r, dtype=np.float32).reshape(-1)
    N = r32.size
    b = bins(t, n_bins, t_lo, t_hi)
    l = loss_value(r32, loss, delta)
    S = np.zeros(n_bins, dtype=np.float64)
    c = np.zeros(n_bins, dtype=np.float64)
    np.add.at(S, b, l)
    np.add.at(c, b, 1.0)
    L = np.where(c > 0, S / np.maximum(c, 1.0), 0.0)
    P = np.cumsum(L) - L  # exclusive prefix
    e = np.float64(np.float32(eps))
    with np.errstate(under="ignore"):
        w_exact = np.exp(-e * P)
        w = w_exact.astype(np.float32).astype(np.float64)
    weighted_sum = float(np.sum(w * S))
    plain_sum = float(np.sum(S))
    rbar = np.float64(np.float32(grad_scale)) * w[b] * loss_derivative(r32, loss, delta)
    return SimpleNamespace(bins=b, S=S, c=c, L=L, P=P, w=w, w_exact=w_exact, weighted_sum=weighted_sum, plain_sum=plain_sum,
                           L_total=weighted_sum / max(N, 1), plain_total=plain_sum / max(N, 1), rbar=rbar)
