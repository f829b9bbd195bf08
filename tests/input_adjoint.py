"""fp64 specification of the input adjoint of the jet streams (what `pinn_jet_backward_inputs` computes).

The K jet streams J = [u, d/dt.., d/dx0..] of a network depend on the coordinates x~ = [x | t] only through its first
stage, so for cotangents c (K, N)

    [xbar | tbar] = d(sum_s c_s J_s)/dx~

is the adjoint of that stage alone:

* coordinate-fed first Linear (feedforward +- LayerNorm, SIREN, ResNet, attention): the derivative streams are seeded with
  constant columns of W, only the value pre-activation z_0 = x~ W^T + b moves with x~, so  [xbar | tbar] = zbar_0 W
  (`linear_input_adjoint`);
* Fourier features phi = [sin p | cos p], p = x~ B (no 2 pi): along a direction with column w of B the feature jets are
  phi_k = f^(k)(p) w^k, so  pbar = sum_s phibar_s f^(k_s + 1)(p) w_s^k_s  and  [xbar | tbar] = pbar B^T
  (`fourier_input_adjoint`).

`jets64` / `input_grads_autograd` are the reference: autograd-of-autograd through `oracle.network_forward`.
"""

from __future__ import annotations

import contextlib
from typing import List, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor


def jets64(spec, sd, x: Tensor, t: Tensor, nt: int, nx: int, layer_norm: str = "composite") -> List[Tensor]:
    """[u, u_t, .., u_x, ..] ((N,) each, x-derivatives along column 0) with the graph kept (x, t require grad)."""
    import oracle as O

    u = O.network_forward(spec, sd, torch.cat([x, t], 1), layer_norm=layer_norm)
    out, cur = [u[:, 0]], u
    for _ in range(nt):
        cur = torch.autograd.grad(cur, t, torch.ones_like(cur), create_graph=True)[0]
        out.append(cur[:, 0])
    cur = u
    for _ in range(nx):
        cur = torch.autograd.grad(cur, x, torch.ones_like(cur), create_graph=True)[0][:, 0:1]
        out.append(cur[:, 0])
    return out


def weighted(J: List[Tensor], cot: Tensor) -> Tensor:
    return sum((cot[s] * J[s]).sum() for s in range(len(J)))


def leaves(x: Tensor, t: Tensor) -> Tuple[Tensor, Tensor]:
    return x.detach().double().clone().requires_grad_(True), t.detach().double().clone().requires_grad_(True)


def input_grads_autograd(spec, sd, x: Tensor, t: Tensor, nt: int, nx: int, cot: Tensor) -> Tuple[Tensor, Tensor]:
    """Reference (xbar (N, dim), tbar (N, 1)) in fp64."""
    sd = {k: v.double() for k, v in sd.items()}
    x, t = leaves(x, t)
    J = jets64(spec, sd, x, t, nt, nx)
    gx, gt = torch.autograd.grad(weighted(J, cot.double()), (x, t))
    return gx, gt


# ---- the specification ------------------------------------------------------------------------------------------
def linear_input_adjoint(W: Tensor, zbar0: Tensor) -> Tuple[Tensor, Tensor]:
    """First Linear (H x din) and the cotangent of its value pre-activation (N, H) -> (xbar, tbar)."""
    g = zbar0 @ W
    return g[:, :-1], g[:, -1:]


def fourier_feature_jets(B: Tensor, xt: Tensor, nt: int, nx: int) -> Tensor:
    """(K, N, 2M) jets of [sin p | cos p] along t (column din - 1 of x~) and x0 (column 0)."""
    p = xt @ B
    f = [torch.sin(p), torch.cos(p), -torch.sin(p), -torch.cos(p)]  # sin^(k) = f[k % 4]; cos^(k) = f[(k + 1) % 4]
    def d(k):
        return torch.cat([f[k % 4], f[(k + 1) % 4]], 1)
    wt, wx = torch.cat([B[-1], B[-1]]), torch.cat([B[0], B[0]])
    out = [d(0)] + [d(k) * wt ** k for k in range(1, nt + 1)] + [d(k) * wx ** k for k in range(1, nx + 1)]
    return torch.stack(out)


def fourier_input_adjoint(B: Tensor, xt: Tensor, phibar: Tensor, nt: int, nx: int) -> Tuple[Tensor, Tensor]:
    """B (din x M), x~ (N x din), phibar (K, N, 2M) cotangents of the feature jets -> (xbar, tbar)."""
    M = B.shape[1]
    p = xt @ B
    f = [torch.sin(p), torch.cos(p), -torch.sin(p), -torch.cos(p)]
    def d(k):  # f^(k) of [sin | cos]
        return torch.cat([f[k % 4], f[(k + 1) % 4]], 1)
    wt, wx = torch.cat([B[-1], B[-1]]), torch.cat([B[0], B[0]])
    pb = phibar[0] * d(1)
    for k in range(1, nt + 1):
        pb = pb + phibar[k] * d(k + 1) * wt ** k
    for k in range(1, nx + 1):
        pb = pb + phibar[nt + k] * d(k + 1) * wx ** k
    pbar = pb[:, :M] + pb[:, M:]  # sin and cos features share the projection column
    g = pbar @ B.T
    return g[:, :-1], g[:, -1:]


# ---- helpers that expose the intermediate cotangents to autograd (tests only) -------------------------------------
@contextlib.contextmanager
def capture_first_linear():
    """Records the output of the first F.linear call made inside the block (the network's first Linear)."""
    orig = F.linear
    box: List[Tensor] = []

    def hooked(inp, w, b=None):
        y = orig(inp, w, b)
        if not box:
            box.append(y)
        return y

    F.linear = hooked
    try:
        yield box
    finally:
        F.linear = orig


def first_linear_cotangent(spec, sd, x: Tensor, t: Tensor, nt: int, nx: int, cot: Tensor) -> Tensor:
    """zbar_0 = d(sum_s c_s J_s)/dz_0 in fp64, z_0 the value pre-activation of the first Linear (through every stream)."""
    sd = {k: v.double() for k, v in sd.items()}
    x, t = leaves(x, t)
    with capture_first_linear() as box:
        J = jets64(spec, sd, x, t, nt, nx)
    return torch.autograd.grad(weighted(J, cot.double()), box[0])[0]


def fourier_feature_cotangent(spec, sd, x: Tensor, t: Tensor, nt: int, nx: int, cot: Tensor) -> Tensor:
    """phibar (K, N, 2M) in fp64: the feature jets are made leaves phi_s, the network after the features is evaluated on
    phi(tau_t, tau_x) = phi_0 + sum_k phi_t,k tau_t^k / k! + sum_k phi_x,k tau_x^k / k!, and its pure tau-derivatives at 0
    are the output jets (they read only the pure coefficients)."""
    import math

    sd = {k: v.double() for k, v in sd.items()}
    B = sd["model.fourier.B"]
    xt = torch.cat([x, t], 1).double()
    phi = fourier_feature_jets(B, xt, nt, nx).detach().requires_grad_(True)
    N = xt.shape[0]
    tt = torch.zeros(N, 1, dtype=torch.float64, requires_grad=True)
    tx = torch.zeros(N, 1, dtype=torch.float64, requires_grad=True)
    z = phi[0]
    for k in range(1, nt + 1):
        z = z + phi[k] * tt ** k / math.factorial(k)
    for k in range(1, nx + 1):
        z = z + phi[nt + k] * tx ** k / math.factorial(k)
    act = {"tanh": torch.tanh, "sin": torch.sin, "gelu": F.gelu, "sigmoid": torch.sigmoid, "relu": F.relu}[spec.activation]
    n = spec.num_layers
    for i in range(n - 1):
        z = act(F.linear(z, sd[f"model.layers.{i}.weight"], sd[f"model.layers.{i}.bias"]))
    u = F.linear(z, sd[f"model.layers.{n - 1}.weight"], sd[f"model.layers.{n - 1}.bias"])
    J, cur = [u[:, 0]], u
    for _ in range(nt):
        cur = torch.autograd.grad(cur, tt, torch.ones_like(cur), create_graph=True)[0]
        J.append(cur[:, 0])
    cur = u
    for _ in range(nx):
        cur = torch.autograd.grad(cur, tx, torch.ones_like(cur), create_graph=True)[0]
        J.append(cur[:, 0])
    return torch.autograd.grad(weighted(J, cot.double()), phi)[0]
