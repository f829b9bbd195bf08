"""`LBFGSDriver` — the control flow of `torch.optim.LBFGS.step()` and of its strong-Wolfe line search on SCALARS.

torch's optimiser (torch/optim/lbfgs.py) mixes two things: decisions taken on a handful of numbers (loss, g.d, max|g|,
sum|g|, max|d|) and arithmetic on n-vectors (the closure, the two-loop recursion, x0 + t d).  The driver keeps the first
and leaves the second to a backend, which on the device is a few launches over flat buffers (`PDETrainer`: the launch
list of the training step without its optimiser tail, `pinn_lbfgs_eval_stats`, `pinn_lbfgs_direction`).  Everything that
decides is restated from torch line by line: `max_iter`, `max_eval`, `tolerance_grad`, `tolerance_change`, the learning
rate read at each `step()`, the first iteration's step `min(1, 1 / sum|g|) lr`, the break conditions in torch's order, the
fixed-step branch of `line_search_fn=None`, and the state (`n_iter`, `func_evals`, `t`, `prev_loss`) carried across
`step()` calls.

The backend is an object with these callables (no tensors cross the interface, so a CPU model can stand in for the device):

    evaluate(t)     closure at x0 + t d (t None: at the current point; no snapshot needed); the gradient it leaves is the
                    "fresh" one.  Returns {"loss", "gtd" (= g.d), "gmax", "gsum"}
    direction(t)    direction update from the current gradient with the previous step length t (ignored on the very first
                    iteration).  Returns {"gtd", "gmax", "gsum", "dmax", "accepted", "count"}
    snapshot()      x0 = current point
    accept(t)       current point = x0 + t d
    save(slot)      keep the fresh gradient in slot 0, 1 or 2
    restore(slot)   make the kept gradient the current one
    reset()         forget the history (n_iter = 0)

A device backend blocks once per `evaluate` and once per `direction`, on one small copy; nothing else is read.
The line search holds on to the gradients of its bracket ends — torch returns `bracket_g[low_pos]`, which need not be the
last evaluation — through three rotating slots: at any time at most the two bracket ends and one more are alive.
"""

from __future__ import annotations

import math
from typing import Callable, Optional

FRESH = -1  # handle of the gradient the last `evaluate` left; 0, 1, 2: a slot


def cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds=None):
    """torch/optim/lbfgs.py:12-37 on Python floats."""
    if bounds is not None:
        xmin_bound, xmax_bound = bounds
    else:
        xmin_bound, xmax_bound = (x1, x2) if x1 <= x2 else (x2, x1)
    d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
    d2_square = d1**2 - g1 * g2
    if d2_square >= 0:
        d2 = math.sqrt(d2_square)
        if x1 <= x2:
            min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
        else:
            min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2))
        return min(max(min_pos, xmin_bound), xmax_bound)
    return (xmin_bound + xmax_bound) / 2.0


class LBFGSDriver:
    def __init__(self, backend, max_iter: int = 20, max_eval: Optional[int] = None, tolerance_grad: float = 1e-7,
                 tolerance_change: float = 1e-9, line_search_fn: Optional[str] = None,
                 lr: Callable[[], float] = lambda: 1.0):
        if line_search_fn not in (None, "strong_wolfe"):
            raise RuntimeError("only 'strong_wolfe' is supported")
        self.backend = backend
        self.max_iter = int(max_iter)
        self.max_eval = int(max_eval) if max_eval is not None else self.max_iter * 5 // 4
        self.tolerance_grad, self.tolerance_change = float(tolerance_grad), float(tolerance_change)
        self.line_search_fn = line_search_fn
        self.lr = lr
        self.n_iter = 0
        self.func_evals = 0
        self.t = None
        self.prev_loss = None

    def reset(self):
        """An empty history, as a freshly constructed torch.optim.LBFGS has."""
        self.n_iter, self.func_evals, self.t, self.prev_loss = 0, 0, None, None
        self.backend.reset()

    # ------------------------------------------------------------------ torch/optim/lbfgs.py:40-209
    def _keep(self, *alive):
        """The fresh gradient into a slot none of the handles `alive` uses."""
        slot = next(s for s in (0, 1, 2) if s not in alive)
        self.backend.save(slot)
        return slot

    def _strong_wolfe(self, t, f, gtd, gmax, d_norm, max_ls, c1=1e-4, c2=0.9):
        B, tolerance_change = self.backend, self.tolerance_change
        g = self._keep()  # torch: g = g.clone(); the first evaluation overwrites the current gradient
        G = {g: gmax}  # max|g| of every kept gradient, for the caller's optimality test
        rec = B.evaluate(t)
        f_new, gtd_new, g_new = rec["loss"], rec["gtd"], FRESH
        G[FRESH] = rec["gmax"]
        ls_func_evals = 1

        t_prev, f_prev, g_prev, gtd_prev = 0, f, g, gtd
        done = False
        ls_iter = 0
        while ls_iter < max_ls:
            if f_new > (f + c1 * t * gtd) or (ls_iter > 1 and f_new >= f_prev):
                bracket = [t_prev, t]
                bracket_f = [f_prev, f_new]
                bracket_g = [g_prev, self._keep(g, g_prev)]
                G[bracket_g[1]] = G[FRESH]
                bracket_gtd = [gtd_prev, gtd_new]
                break

            if abs(gtd_new) <= -c2 * gtd:
                bracket = [t]
                bracket_f = [f_new]
                bracket_g = [g_new]
                done = True
                break

            if gtd_new >= 0:
                bracket = [t_prev, t]
                bracket_f = [f_prev, f_new]
                bracket_g = [g_prev, self._keep(g, g_prev)]
                G[bracket_g[1]] = G[FRESH]
                bracket_gtd = [gtd_prev, gtd_new]
                break

            min_step = t + 0.01 * (t - t_prev)
            max_step = t * 10
            tmp = t
            t = cubic_interpolate(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, bounds=(min_step, max_step))

            t_prev = tmp
            f_prev = f_new
            g_prev = self._keep(g)  # the previous g_prev is dropped (the initial g stays: it is needed at max_ls)
            G[g_prev] = G[FRESH]
            gtd_prev = gtd_new
            rec = B.evaluate(t)
            f_new, gtd_new = rec["loss"], rec["gtd"]
            G[FRESH] = rec["gmax"]
            ls_func_evals += 1
            ls_iter += 1

        if ls_iter == max_ls:
            bracket = [0, t]
            bracket_f = [f, f_new]
            bracket_g = [g, g_new]

        insuf_progress = False
        low_pos, high_pos = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0)
        while not done and ls_iter < max_ls:
            if abs(bracket[1] - bracket[0]) * d_norm < tolerance_change:
                break

            t = cubic_interpolate(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1])

            eps = 0.1 * (max(bracket) - min(bracket))
            if min(max(bracket) - t, t - min(bracket)) < eps:
                if insuf_progress or t >= max(bracket) or t <= min(bracket):
                    if abs(t - max(bracket)) < abs(t - min(bracket)):
                        t = max(bracket) - eps
                    else:
                        t = min(bracket) + eps
                    insuf_progress = False
                else:
                    insuf_progress = True
            else:
                insuf_progress = False

            rec = B.evaluate(t)
            f_new, gtd_new = rec["loss"], rec["gtd"]
            G[FRESH] = rec["gmax"]
            ls_func_evals += 1
            ls_iter += 1

            if f_new > (f + c1 * t * gtd) or f_new >= bracket_f[low_pos]:
                bracket[high_pos] = t
                bracket_f[high_pos] = f_new
                bracket_g[high_pos] = self._keep(bracket_g[low_pos])
                G[bracket_g[high_pos]] = G[FRESH]
                bracket_gtd[high_pos] = gtd_new
                low_pos, high_pos = (0, 1) if bracket_f[0] <= bracket_f[1] else (1, 0)
            else:
                if abs(gtd_new) <= -c2 * gtd:
                    done = True
                elif gtd_new * (bracket[high_pos] - bracket[low_pos]) >= 0:
                    bracket[high_pos] = bracket[low_pos]
                    bracket_f[high_pos] = bracket_f[low_pos]
                    bracket_g[high_pos] = bracket_g[low_pos]
                    bracket_gtd[high_pos] = bracket_gtd[low_pos]

                bracket[low_pos] = t
                bracket_f[low_pos] = f_new
                bracket_g[low_pos] = self._keep(bracket_g[high_pos])
                G[bracket_g[low_pos]] = G[FRESH]
                bracket_gtd[low_pos] = gtd_new

        t = bracket[low_pos]
        f_new = bracket_f[low_pos]
        g_new = bracket_g[low_pos]
        return f_new, g_new, G[g_new], t, ls_func_evals

    # ------------------------------------------------------------------ torch/optim/lbfgs.py:332-537
    def step(self) -> float:
        """One `optimizer.step(closure)`.  Returns the loss of its first evaluation, as torch does."""
        B = self.backend
        lr = float(self.lr())
        max_iter, max_eval = self.max_iter, self.max_eval
        tolerance_grad, tolerance_change = self.tolerance_grad, self.tolerance_change

        rec = B.evaluate(None)
        orig_loss = loss = rec["loss"]
        current_evals = 1
        self.func_evals += 1
        if rec["gmax"] <= tolerance_grad:
            return orig_loss

        t, prev_loss = self.t, self.prev_loss
        n_iter = 0
        while n_iter < max_iter:
            n_iter += 1
            self.n_iter += 1

            drec = B.direction(t if t is not None else 0.0)  # memory update + two-loop recursion; prev_grad = g
            prev_loss = loss

            if self.n_iter == 1:
                t = min(1.0, 1.0 / drec["gsum"]) * lr
            else:
                t = lr

            gtd = drec["gtd"]
            if gtd > -tolerance_change:
                break

            ls_func_evals = 0
            if self.line_search_fn is not None:
                B.snapshot()
                loss, g_new, gmax, t, ls_func_evals = self._strong_wolfe(t, loss, gtd, drec["gmax"], drec["dmax"],
                                                                         max_eval - current_evals)
                if g_new != FRESH:
                    B.restore(g_new)
                B.accept(t)
                opt_cond = gmax <= tolerance_grad
            else:
                B.snapshot()
                B.accept(t)
                opt_cond = False  # torch keeps the flag of the step's first evaluation here, which was False
                if n_iter != max_iter:
                    rec = B.evaluate(None)
                    loss = rec["loss"]
                    opt_cond = rec["gmax"] <= tolerance_grad
                    ls_func_evals = 1

            current_evals += ls_func_evals
            self.func_evals += ls_func_evals

            if n_iter == max_iter:
                break
            if current_evals >= max_eval:
                break
            if opt_cond:
                break
            if drec["dmax"] * abs(t) <= tolerance_change:
                break
            if abs(loss - prev_loss) < tolerance_change:
                break

        self.t, self.prev_loss = t, prev_loss
        return orig_loss
