"""The unimodular shear of a jet launch along a direction (PINN_FLAG_SPACE_DIRECTION, include/pinn_jet.h) as the tests use it.

With p the first axis of the direction d (d_p = +1) and s(.) the exchange of columns 0 and p, the sheared network sees
    x'_0 = x_p,   x'_j = x_s(j) - d_s(j) x_p   (j != 0),   t untouched,
through the coordinate map
    W'[:,0] = W[:,p] + sum_{c != p} d_c W[:,c],   W'[:,j] = W[:,s(j)],
so u'(x') = u(x) and d^k u' / dx'_0^k = (sum_c d_c d/dx_c)^k u: the axis-0 jets of the sheared network, from
tests/jet_model.py, ARE the directional derivatives.  In the dtype of its arguments: fp64 tensors give the exact shear of
fp32 numbers (every sum of two or three fp32 numbers is exact in fp64), fp32 tensors the engine's own numbers bit for bit —
one add or subtract per entry, in ascending c.  The gradients come back through the transposes."""

import torch


def pivot(direction):
    return next(c for c, v in enumerate(direction) if v != 0)


def _sigma(j, p):
    return p if j == 0 else (0 if j == p else j)


def _entries(direction, n):
    """d_c per column of an n-column map or input, the pivot's own entry and everything beyond the direction zero."""
    p = pivot(direction)
    return [direction[c] if (c < len(direction) and c != p) else 0 for c in range(n)]


def shear_inputs(inp, direction):
    """inp (N, din) = [x | t] -> the coordinates the sheared network reads."""
    p, d = pivot(direction), _entries(direction, inp.shape[1])
    cols = []
    for j in range(inp.shape[1]):
        c = _sigma(j, p)
        col = inp[:, c]
        if j != 0 and d[c] != 0:
            col = col - inp[:, p] if d[c] > 0 else col + inp[:, p]
        cols.append(col)
    return torch.stack(cols, dim=1)


def shear_map(W, direction, fourier):
    """The coordinate map (first Linear (H, din), or Fourier B (din, M)) of the sheared network."""
    Wc = W.t() if fourier else W  # (rows, din): one column per coordinate
    p, d = pivot(direction), _entries(direction, Wc.shape[1])
    cols = []
    for j in range(Wc.shape[1]):
        col = Wc[:, _sigma(j, p)]
        if j == 0:
            for c in range(Wc.shape[1]):
                if d[c] != 0:
                    col = col + Wc[:, c] if d[c] > 0 else col - Wc[:, c]
        cols.append(col)
    out = torch.stack(cols, dim=1)
    return out.t().contiguous() if fourier else out.contiguous()


def shear_state_dict(sd, first, direction):
    out = dict(sd)
    out[first] = shear_map(sd[first], direction, first.endswith("fourier.B"))
    return out


def unshear_map_grad(g, direction):
    """Gradient of a first Linear (H, din) of the sheared network -> gradient of the network as given."""
    p, d = pivot(direction), _entries(direction, g.shape[1])
    cols = []
    for c in range(g.shape[1]):
        col = g[:, _sigma(c, p)]
        if d[c] != 0:
            col = col + g[:, 0] if d[c] > 0 else col - g[:, 0]
        cols.append(col)
    return torch.stack(cols, dim=1)


def unshear_input_grad(ig, direction):
    """Cotangent of the sheared coordinates (N, din) -> cotangent of [x | t] as given."""
    p, d = pivot(direction), _entries(direction, ig.shape[1])
    cols = []
    for c in range(ig.shape[1]):
        col = ig[:, _sigma(c, p)]
        if c == p:
            for a in range(ig.shape[1]):
                if d[a] != 0:
                    col = col - ig[:, _sigma(a, p)] if d[a] > 0 else col + ig[:, _sigma(a, p)]
        cols.append(col)
    return torch.stack(cols, dim=1)
