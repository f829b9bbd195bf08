"""fp64 models of the training-step kernels (csrc/train_kernels.hip): the point-wise loss terms of `pinn_jet_losses` /
`pinn_point_losses` and clip + Adam of `pinn_adam_clip_step`.  The loss comes from `oracle.apply_loss_fn` and the cotangent
from autograd; the optimiser is `adaptive_model.FlatAdam` with one component of weight 1.  No product code.

`AdamFp32` is NOT a model: it is the specified optimiser arithmetic (torch's Adam, bias corrections as
-expm1(t log beta)) evaluated in numpy fp32, the yardstick for what fp32 can deliver on given inputs."""

import numpy as np
import torch

import oracle as O
from adaptive_model import FlatAdam


def jet_loss_terms(jets64, terms, loss, huber_delta, residual_sum=None, residual_scale=0.0, residual_weight=0.0,
                   n_boundary_terms=0):
    """jets64: (K, n).  term k = (lo, hi, stream, pair_offset, target | None, weight), as `engine.jet_losses` takes them:
    term_k = mean l(J[stream, lo:hi] - target) or, pair_offset != 0, mean l(J[stream, lo:hi] - J[stream, lo+pair : hi+pair]).
    An empty term (lo == hi) is 0 and has no cotangent (the kernels' convention; torch's mean of nothing is NaN).

    Returns (term_losses (n_terms,), cot (K, n) = d sum_k weight_k term_k / d jets, summary4 = {residual, boundary, initial,
    total} with residual = residual_sum * residual_scale, boundary = the first n_boundary_terms terms, initial = the rest,
    total = residual_weight * residual + sum_k weight_k term_k), numpy fp64."""
    J = torch.as_tensor(np.asarray(jets64, dtype=np.float64)).clone().requires_grad_(True)
    vals = []
    for lo, hi, stream, pair, target, _ in terms:
        if hi == lo:
            vals.append(J.sum() * 0.0)
            continue
        other = J[stream, lo + pair : hi + pair] if pair else torch.as_tensor(np.asarray(target, dtype=np.float64))
        vals.append(O.apply_loss_fn(J[stream, lo:hi] - other, loss, float(huber_delta)))
    weights = [float(t[5]) for t in terms]
    weighted = sum((w * v for w, v in zip(weights, vals)), J.sum() * 0.0)
    (cot,) = torch.autograd.grad(weighted, J)
    L = np.array([float(v.detach()) for v in vals], dtype=np.float64)
    res = float(residual_sum) * float(residual_scale) if residual_sum is not None else 0.0
    summary = np.array([res, L[:n_boundary_terms].sum(), L[n_boundary_terms:].sum(), float(residual_weight) * res + float(weighted.detach())])
    return L, cot.numpy(), summary


def point_loss_terms(u64, terms, loss, huber_delta, **kw):
    """`engine.point_losses`' terms (lo, hi, target, weight) on one row of values: the K = 1 case of `jet_loss_terms`."""
    L, cot, summary = jet_loss_terms(np.asarray(u64, dtype=np.float64)[None, :], [(lo, hi, 0, 0, tg, w) for lo, hi, tg, w in terms],
                                     loss, huber_delta, **kw)
    return L, cot[0], summary


def r32(x):
    """The number an fp32 argument of the C ABI carries."""
    return float(np.float32(x))


def make_adam(n, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0, m=None, v=None, t=0):
    """FlatAdam from theta = 0 with the hyper-parameters rounded to fp32 as `pinn_adam_clip_step` takes them
    (1 - beta2 of the rounded 0.999 is 1.3e-5 away from 1e-3); optional preset moments and step count."""
    a = FlatAdam(np.zeros(n), lr=r32(lr), beta1=r32(beta1), beta2=r32(beta2), eps=r32(eps), weight_decay=r32(weight_decay),
                 max_norm=float(max_norm))
    if m is not None:
        a.m = np.asarray(m, dtype=np.float64).copy()
    if v is not None:
        a.v = np.asarray(v, dtype=np.float64).copy()
    a.t = int(t)
    return a


def adam_step(adam, g):
    """One clip + Adam step on the gradient g (n,): one component, weight 1.  Returns the norm before clipping."""
    return adam.step(np.asarray(g, dtype=np.float64)[None, :], [1.0])[1]


class AdamFp32:
    """The specified arithmetic in numpy fp32: clip_grad_norm_ + torch's Adam, bc = -expm1(t log beta)."""

    def __init__(self, n, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0, m=None, v=None, t=0):
        f = np.float32
        self.theta = np.zeros(n, dtype=f)
        self.m = np.zeros(n, dtype=f) if m is None else np.asarray(m, dtype=f).copy()
        self.v = np.zeros(n, dtype=f) if v is None else np.asarray(v, dtype=f).copy()
        self.t = f(t)
        self.lr, self.b1, self.b2, self.eps, self.wd, self.max_norm = f(lr), f(beta1), f(beta2), f(eps), f(weight_decay), f(max_norm)

    def step(self, g):
        f = np.float32
        g = np.asarray(g, dtype=f)
        norm = np.sqrt(np.sum(g * g, dtype=f), dtype=f)
        gi = g
        if self.max_norm > 0:
            gi = g * min(f(1.0), self.max_norm / (norm + f(1e-6)))
        if self.wd != 0:
            gi = gi + self.wd * self.theta
        self.t = f(self.t + f(1.0))
        self.m = self.m + (f(1.0) - self.b1) * (gi - self.m)
        self.v = self.b2 * self.v + (f(1.0) - self.b2) * gi * gi
        bc1 = -np.expm1(self.t * np.log(self.b1))
        bc2 = -np.expm1(self.t * np.log(self.b2))
        denom = np.sqrt(self.v) / np.sqrt(bc2) + self.eps
        self.theta = self.theta - (self.lr / bc1) * (self.m / denom)
        assert self.theta.dtype == self.m.dtype == self.v.dtype == f and isinstance(bc1, f) and isinstance(norm, f)
        return float(norm)


def rel_l2_np(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    d = a - b
    return float(np.sqrt(np.sum(d * d)) / max(float(np.sqrt(np.sum(b * b))), 1e-30))
