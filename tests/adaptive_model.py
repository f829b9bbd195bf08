"""fp64 restatements used by the adaptive-weight tests: the two EMA weight rules (RBW / LRW) and "combine the component
gradients with the weights, clip, Adam" on flat arrays.  Plain numpy, no product code."""

import numpy as np


class EmaWeights:
    """v = loss magnitudes (rbw) or gradient norms (lrw), one entry per component.

    First call: running = v; the weights are `initial_weights` (ones when None).  Later calls:
    running = alpha running + (1 - alpha) v;  lrw: w = inv / sum(inv), inv = 1 / (running + eps);
    rbw: w = running / (sum(running) + eps), and from the third call on w = alpha prev + (1 - alpha) w (prev = the rbw
    weights of the call before, which the first call does not set)."""

    def __init__(self, strategy, alpha, eps, initial_weights=None):
        assert strategy in ("rbw", "lrw")
        self.strategy, self.alpha, self.eps = strategy, float(alpha), float(eps)
        self.initial = None if initial_weights is None else np.asarray(initial_weights, dtype=np.float64)
        self.running = self.prev = self.weights = None

    def update(self, v):
        v = np.asarray(v, dtype=np.float64)
        if self.running is None:
            self.running = v.copy()
            self.weights = self.initial.copy() if self.initial is not None else np.ones_like(v)
            return self.weights
        self.running = self.alpha * self.running + (1.0 - self.alpha) * v
        if self.strategy == "lrw":
            inv = 1.0 / (self.running + self.eps)
            self.weights = inv / inv.sum()
        else:
            w = self.running / (self.running.sum() + self.eps)
            if self.prev is not None:
                w = self.alpha * self.prev + (1.0 - self.alpha) * w
            self.prev = w.copy()
            self.weights = w
        return self.weights

    def state16(self):
        """The device state of pinn_adaptive_adam_step: {running[4], prev_weights[4], weights[4], calls != 0, has_prev}."""
        s = np.zeros(14)
        if self.running is not None:
            c = len(self.running)
            s[0:c], s[8 : 8 + c], s[12] = self.running, self.weights, 1.0
            if self.prev is not None:
                s[4 : 4 + c], s[13] = self.prev, 1.0
        return s


class FlatAdam:
    """torch.nn.utils.clip_grad_norm_(max_norm) + torch.optim.Adam(lr, betas, eps, weight_decay) on one flat fp64 array."""

    def __init__(self, theta, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0):
        self.theta = np.asarray(theta, dtype=np.float64).copy()
        self.m, self.v, self.t = np.zeros_like(self.theta), np.zeros_like(self.theta), 0
        self.lr, self.b1, self.b2, self.eps, self.wd, self.max_norm = lr, beta1, beta2, eps, weight_decay, max_norm

    def step(self, comp_grads, weights):
        """comp_grads: (C, n); weights: (C,).  Returns (combined gradient before clipping, its norm)."""
        g = (np.asarray(weights, dtype=np.float64)[:, None] * np.asarray(comp_grads, dtype=np.float64)).sum(0)
        norm = float(np.sqrt((g * g).sum()))
        gi = g * min(1.0, self.max_norm / (norm + 1e-6)) if self.max_norm > 0 else g.copy()
        if self.wd:
            gi = gi + self.wd * self.theta
        self.t += 1
        self.m = self.b1 * self.m + (1.0 - self.b1) * gi
        self.v = self.b2 * self.v + (1.0 - self.b2) * gi * gi
        denom = np.sqrt(self.v) / np.sqrt(1.0 - self.b2**self.t) + self.eps
        self.theta = self.theta - self.lr / (1.0 - self.b1**self.t) * self.m / denom
        return g, norm


def adaptive_step(rule, adam, comp_grads, comp_losses):
    """One step of the adaptive-weight launch list on flat arrays: (weights, summary4, norm before clipping, combined g)."""
    comp_grads = np.asarray(comp_grads, dtype=np.float64)
    L = np.asarray(comp_losses, dtype=np.float64)
    v = np.sqrt((comp_grads * comp_grads).sum(1)) if rule.strategy == "lrw" else L
    w = rule.update(v).copy()
    g, norm = adam.step(comp_grads, w)
    summary = np.zeros(4)
    summary[: min(3, len(L))] = L[:3]
    summary[3] = float((w * L).sum())
    return w, summary, norm, g
