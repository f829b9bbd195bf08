"""Executable model of the MERGED stream set of `csrc/jet_device.h` (closed-form, no autograd).

A residual that reads u_t and u_xx only through w = u_t + c u_xx = D u, D = d/dt + c d2/dx2, needs the three streams
[value, w, d/dx] instead of the four [value, d/dt, d/dx, d2/dx2]:

  * Linear layer:  D(W a + b) = W (D a)
  * activation y = f(z):  y_x = f' z_x,  y_w = f' z_w + c f'' z_x^2
  * adjoint:  zb_w = f' yb_w;  zb_x = f' yb_x + 2 c f'' z_x yb_w;
              zb_0 = f' yb_0 + f'' z_x yb_x + (f'' z_w + c f''' z_x^2) yb_w
  * dL/dc = sum over every activation element (Fourier features included) of yb_w f'' z_x^2

Burgers: c = -nu, r = w + u u_x, dL/dnu = -dL/dc.  The programs are those of `jet_model.mlp_program`; the stream order
[value, w, x] is the (1,1) order with w in the time slot, which is how the kernels lay the set out.
"""

from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

import jet_model as J

Tensor = torch.Tensor


def act_fwd(act: str, param: float, c: float, z: List[Tensor]) -> List[Tensor]:
    f = J.act_derivs(act, param, z[0], 2)
    return [f[0], f[1] * z[1] + c * f[2] * z[2] ** 2, f[1] * z[2]]


def act_bwd(act: str, param: float, c: float, z: List[Tensor], ab: List[Tensor]) -> Tuple[List[Tensor], Tensor]:
    """Returns ([zb_0, zb_w, zb_x], the elements' coefficient partials)."""
    f = J.act_derivs(act, param, z[0], 3)
    zx2 = z[2] ** 2
    zb_w = f[1] * ab[1]
    zb_x = f[1] * ab[2] + 2 * c * f[2] * z[2] * ab[1]
    zb_0 = f[1] * ab[0] + f[2] * z[2] * ab[2] + (f[2] * z[1] + c * f[3] * zx2) * ab[1]
    return [zb_0, zb_w, zb_x], ab[1] * f[2] * zx2


def jets_forward(prog: Dict, inp: Tensor, c: float):
    """Jets [u, w, u_x] of the network output and the tape of the reverse sweep."""
    a = J.input_streams(inp, 1, 1)  # D(inp) = e_time: the second derivative of the identity vanishes
    tape = {"z": [], "a_in": [], "enc_z": None}
    if prog["enc"] == "fourier":
        z = [s @ prog["B"] for s in a]
        tape["enc_z"] = z
        sin_j = act_fwd("sin", 1.0, c, z)
        cos_j = act_fwd("sin", 1.0, c, [z[0] + math.pi / 2] + z[1:])
        a = [torch.cat([s, k], -1) for s, k in zip(sin_j, cos_j)]
    for W, b, act, par, _ in prog["hidden"]:
        tape["a_in"].append(a)
        z = [a[0] @ W.T + b] + [a[s] @ W.T for s in (1, 2)]
        tape["z"].append(z)
        a = act_fwd(act, par, c, z)
    Wo, bo, _ = prog["out"]
    tape["a_last"] = a
    return [a[0] @ Wo.T + bo, a[1] @ Wo.T, a[2] @ Wo.T], tape


def jets_backward(prog: Dict, tape: Dict, ubar: List[Tensor], c: float):
    """Returns ({param name: grad}, dL/dc)."""
    g: Dict[str, Tensor] = {}
    Wo, _, no = prog["out"]
    a = tape["a_last"]
    g[no + ".weight"] = sum(ubar[s].T @ a[s] for s in range(3))
    g[no + ".bias"] = ubar[0].sum(0)
    abar = [ubar[s] @ Wo for s in range(3)]
    dc = torch.zeros((), dtype=ubar[0].dtype)
    for li in range(len(prog["hidden"]) - 1, -1, -1):
        W, _, act, par, nm = prog["hidden"][li]
        zb, part = act_bwd(act, par, c, tape["z"][li], abar)
        dc = dc + part.sum()
        a_in = tape["a_in"][li]
        g[nm + ".weight"] = sum(zb[s].T @ a_in[s] for s in range(3))
        g[nm + ".bias"] = zb[0].sum(0)
        abar = [zb[s] @ W for s in range(3)]
    if prog["enc"] == "fourier":  # e = -b_x^2 (value features): the features' own coefficient partial
        z = tape["enc_z"]
        M = z[0].shape[-1]
        _, ps = act_bwd("sin", 1.0, c, z, [s[:, :M] for s in abar])
        _, pc = act_bwd("sin", 1.0, c, [z[0] + math.pi / 2] + z[1:], [s[:, M:] for s in abar])
        dc = dc + ps.sum() + pc.sum()
    return g, dc


def burgers_residual(j: List[Tensor]):
    """r = w + u u_x and dr/d[u, w, u_x]."""
    return j[1] + j[0] * j[2], [j[2], torch.ones_like(j[0]), j[0]]


def burgers_loss_grad(prog: Dict, inp: Tensor, nu: float):
    """(residual, mean-square loss, {param: grad}, dL/dnu) on the merged set."""
    c = -nu
    N = inp.shape[0]
    j, tape = jets_forward(prog, inp, c)
    r, d = burgers_residual(j)
    rb = 2.0 * r / N
    g, dc = jets_backward(prog, tape, [rb * k for k in d], c)
    return r, (r * r).mean(), g, -dc


def burgers_loss_grad_plain(prog: Dict, inp: Tensor, nu: float):
    """The same four results on the four streams of `jet_model` (the reference of the merged form)."""
    N = inp.shape[0]
    j, tape = J.mlp_jets_forward(prog, inp, 1, 2)
    r, d = J.pde_residual("burgers", {"nu": nu}, j, inp[:, :1], 1, 2)
    rb = 2.0 * r / N
    g = J.mlp_jets_backward(prog, tape, [rb * k for k in d], 1, 2)
    return r, (r * r).mean(), g, (rb * -j[3]).sum()
