"""fp64 model of the finite-difference smoothness term on the launch list (csrc/train_kernels.hip: `pinn_fd_stencil_points`,
`pinn_fd_smoothness`; the reference: pinnrl/pdes/heat_equation.py:625-650), 1-D:

    S = mean|(u(x+e,t) - u(x,t))/e| + mean|(u(x,t) - u(x-e,t))/e|,   shifted points clamped to [lo, hi].

`stencil_points` is the specified fp32 arithmetic of the evaluation points (they are inputs of the network: the entry point
has to reproduce them bit for bit); `smoothness_terms` is S and dS/du3 in fp64 from given values; `term_and_weight_gradient`
is the whole term through the fp64 network of `tests/jet_model.py`.  No product code."""

import numpy as np
import torch

import jet_model as JM
import train_step_model as TS

F32 = np.float32


def stencil_points(x32, t32, eps, lo, hi):
    """x3 = [x | clamp(x + e) | clamp(x - e)], t3 = [t | t | t] in numpy fp32: e, lo, hi rounded to fp32, one fp32 add,
    clamp = min(max(v, lo), hi) — what torch.clamp(x + eps, lo, hi) computes on fp32 tensors."""
    x = np.asarray(x32, dtype=F32).ravel()
    t = np.asarray(t32, dtype=F32).ravel()
    e, lo, hi = F32(eps), F32(lo), F32(hi)
    xp = np.minimum(np.maximum(x + e, lo), hi)
    xm = np.minimum(np.maximum(x - e, lo), hi)
    assert xp.dtype == F32 and xm.dtype == F32
    return np.concatenate([x, xp, xm]), np.concatenate([t, t, t])


def smoothness_terms(u3, eps, weight=1.0):
    """u3 = [uc | up | um] (3N values, any float type; taken to fp64 exactly).  Returns (S, cot3) with
    cot3 = weight * dS/du3 = weight / (eps N) * [sgn(uc - um) - sgn(up - uc) | sgn(up - uc) | -sgn(uc - um)], sgn(0) = 0."""
    u = np.asarray(u3, dtype=np.float64).ravel()
    assert u.size % 3 == 0 and u.size > 0
    n = u.size // 3
    uc, up, um = u[:n], u[n : 2 * n], u[2 * n :]
    d1, d2 = up - uc, uc - um
    S = float(np.mean(np.abs(d1 / eps)) + np.mean(np.abs(d2 / eps)))
    s1, s2 = np.sign(d1), np.sign(d2)
    c = float(weight) / (float(eps) * n)
    return S, np.concatenate([(s2 - s1) * c, s1 * c, -s2 * c])


def term_and_weight_gradient(spec, sd, x32, t32, eps, lo, hi, weight=1.0, dtype=torch.float64):
    """The whole term on the fp64 network: stencil points from the fp32 batch, values by `jet_model.program_forward`
    (orders 0, 0), S and cotangents by `smoothness_terms`, weight gradient by `jet_model.program_backward`.
    Returns (S, {parameter name: d(weight * S)/d(parameter)}, u3 (3N,)).  `dtype=torch.float32` runs the same network
    arithmetic in fp32 (a yardstick for what fp32 delivers on given inputs, not a model)."""
    sdx = {k: v.detach().to(dtype) for k, v in sd.items()}
    x3, t3 = stencil_points(x32, t32, eps, lo, hi)
    inp = torch.from_numpy(np.stack([x3, t3], 1)).to(dtype)
    prog = JM.net_program(spec, sdx)
    u, tape = JM.program_forward(prog, inp, 0, 0)
    u3 = u[0].reshape(-1).numpy()
    S, cot = smoothness_terms(u3, eps, weight)
    g = JM.program_backward(prog, tape, [torch.from_numpy(cot).reshape(-1, 1).to(dtype)], 0, 0)
    return S, g, u3


def heat_step(spec, sd, x32, t32, alpha, residual_weight, chain_x, chain_t, terms, n_bc, smooth, has_data=False, dtype=torch.float64):
    """One evaluation of HeatEquation.compute_loss (1-D, mse, fixed weights) on the fp64 network: residual u_t - alpha u_x
    (the reference's heat residual: its "laplacian" is a first derivative) on the batch, the boundary / initial (/ data)
    chain `terms` (as `engine.jet_losses` takes them, on the (u, u_t, u_x) jets of the points chain_x, chain_t), and the
    smoothness term `smooth` = {"eps", "weight", "lo", "hi"} | None.
    Returns ({residual, boundary, initial, smoothness, total[, data]}, {parameter name: d total / d parameter}, d total / d alpha)."""
    sdx = {k: v.detach().to(dtype) for k, v in sd.items()}
    prog = JM.net_program(spec, sdx)
    x = np.asarray(x32, dtype=np.float32).reshape(-1, 1)
    t = np.asarray(t32, dtype=np.float32).reshape(-1, 1)
    n = x.shape[0]
    j, tape = JM.program_forward(prog, torch.from_numpy(np.concatenate([x, t], 1)).to(dtype), 1, 1)
    r = j[1] - alpha * j[2]
    res = float((r.double() ** 2).mean())
    rbar = (2.0 * residual_weight / n) * r
    grads = JM.program_backward(prog, tape, [torch.zeros_like(r), rbar, -alpha * rbar], 1, 1)
    dalpha = float((rbar.double() * -j[2].double()).sum())
    cx = np.asarray(chain_x, dtype=np.float32).reshape(-1, 1)
    ct = np.asarray(chain_t, dtype=np.float32).reshape(-1, 1)
    jc, tape_c = JM.program_forward(prog, torch.from_numpy(np.concatenate([cx, ct], 1)).to(dtype), 1, 1)
    J = np.stack([s.reshape(-1).double().numpy() for s in jc])
    L, cot, summary = TS.jet_loss_terms(J, terms, "mse", 1.0, residual_sum=res * n, residual_scale=1.0 / n,
                                        residual_weight=residual_weight, n_boundary_terms=n_bc)
    gc = JM.program_backward(prog, tape_c, [torch.from_numpy(cot[s]).reshape(-1, 1).to(dtype) for s in range(3)], 1, 1)
    for k in grads:
        grads[k] = grads[k] + gc[k]
    losses = {"residual": summary[0], "boundary": summary[1], "initial": summary[2], "smoothness": 0.0, "total": summary[3]}
    if has_data:
        losses["initial"], losses["data"] = float(L[n_bc:-1].sum()), float(L[-1])
    if smooth is not None:
        S, gs, _ = term_and_weight_gradient(spec, sd, x, t, smooth["eps"], smooth["lo"], smooth["hi"], smooth["weight"], dtype=dtype)
        for k in grads:
            grads[k] = grads[k] + gs[k]
        losses["smoothness"] = S
        losses["total"] = losses["total"] + smooth["weight"] * S
    return {k: float(v) for k, v in losses.items()}, grads, dalpha
