"""fp64 model of the L-BFGS direction update (`pinn_lbfgs_direction`) and of the line search's reductions
(`pinn_lbfgs_eval_stats`): the memory update of torch/optim/lbfgs.py:396-421 with its 1e-10 rejection and the eviction of
the oldest pair, the two-loop recursion of lines 423-442 in VECTOR form, and the fields of the record.  numpy only.

`two_loop(..., dtype=np.float32)` is the same recursion with every vector operation rounded to fp32 as torch's fp32 tensors
round it: the control that sets the bar for the kernel's direction."""

import numpy as np


def two_loop(g, S, Y, ro, h_diag, dtype=np.float64):
    """d = -H g for the pairs (S[i], Y[i]) oldest first (lbfgs.py:432-442).  With dtype float32 the vectors, dots and
    scalars are fp32 throughout, like torch's on fp32 tensors (ro and H_diag are fp32 tensors there too)."""
    f = dtype
    q = (-g).astype(f)
    n_old = len(S)
    al = [None] * n_old
    S = [s.astype(f) for s in S]
    Y = [y.astype(f) for y in Y]
    ro = [f(r) for r in ro]
    for i in range(n_old - 1, -1, -1):
        al[i] = f(np.dot(S[i], q)) * ro[i]
        q = (q + Y[i] * f(-al[i])).astype(f)
    r = (q * f(h_diag)).astype(f)
    for i in range(n_old):
        be = f(np.dot(Y[i], r)) * ro[i]
        r = (r + S[i] * f(al[i] - be)).astype(f)
    return r


class LBFGSModel:
    """State of one torch.optim.LBFGS (direction part) in double.  Inputs are taken as given (fp32 values stay exactly
    what they are); nothing is rounded."""

    def __init__(self, history_size):
        self.history_size = int(history_size)
        self.reset()

    def reset(self):
        self.S, self.Y, self.ro = [], [], []
        self.h_diag = 1.0
        self.n_iter = 0
        self.prev_grad = None
        self.d = None

    def direction(self, g, t_prev=0.0, pair=None):
        """One update.  The tentative pair is (s = t_prev d, y = g - prev_grad), or `pair` = (s, y) when the caller has the
        pair the device formed (fp32-rounded).  Returns the record as a dict; `self.d` is the new direction."""
        g = np.asarray(g, dtype=np.float64)
        accepted = False
        if self.n_iter == 0:
            self.S, self.Y, self.ro, self.h_diag = [], [], [], 1.0
            d = -g
        else:
            if pair is None:
                s, y = float(t_prev) * self.d, g - self.prev_grad
            else:
                s, y = np.asarray(pair[0], dtype=np.float64), np.asarray(pair[1], dtype=np.float64)
            ys = float(np.dot(y, s))
            if ys > 1e-10:
                accepted = True
                if len(self.S) == self.history_size:
                    self.S.pop(0), self.Y.pop(0), self.ro.pop(0)
                self.S.append(s), self.Y.append(y), self.ro.append(1.0 / ys)
                self.h_diag = ys / float(np.dot(y, y))
            d = two_loop(g, self.S, self.Y, self.ro, self.h_diag)
        self.n_iter += 1
        self.prev_grad = g.copy()
        self.d = d
        return {"loss": 0.0, "gtd": float(np.dot(g, d)), "gmax": float(np.abs(g).max()), "gsum": float(np.abs(g).sum()),
                "dmax": float(np.abs(d).max()), "accepted": accepted, "count": len(self.S), "n_iter": self.n_iter,
                "h_diag": float(self.h_diag)}


def eval_stats(g, d, loss):
    g, d = np.asarray(g, dtype=np.float64), np.asarray(d, dtype=np.float64)
    return {"loss": float(loss), "gtd": float(np.dot(g, d)), "gmax": float(np.abs(g).max()), "gsum": float(np.abs(g).sum())}


class ModelBackend:
    """`LBFGSDriver` backend over `LBFGSModel` and a Python objective `fun(x) -> (loss, grad)` in double: what the device
    backend of `PDETrainer` does with launches, on numpy arrays."""

    def __init__(self, fun, x, history_size):
        self.fun, self.x = fun, np.array(x, dtype=np.float64)
        self.model = LBFGSModel(history_size)
        self.x0 = self.x.copy()
        self.g = np.zeros_like(self.x)
        self.slots = [None, None, None]
        self.evals = 0

    def reset(self):
        self.model.reset()

    def evaluate(self, t):
        if t is not None:
            self.x = self.x0 + t * self.model.d
        loss, g = self.fun(self.x)
        self.g = np.asarray(g, dtype=np.float64)
        self.evals += 1
        d = self.model.d if self.model.d is not None else np.zeros_like(self.g)
        return eval_stats(self.g, d, loss)

    def direction(self, t_prev):
        return self.model.direction(self.g, t_prev)

    def snapshot(self):
        self.x0 = self.x.copy()

    def accept(self, t):
        self.x = self.x0 + t * self.model.d

    def save(self, slot):
        self.slots[slot] = self.g.copy()

    def restore(self, slot):
        self.g = self.slots[slot].copy()
