"""fp64 model of the activation jets of `pinns-rl-pde_amd/csrc/jet_device.h`, with a per-element error bound for every output.

Test infrastructure for tests/test_jet_device_gpu.py (the HIP text of the header, element by element, through the probe library)
and tests/test_jet_device_model_cpu.py (this model against mpmath, an fp32 emulation against the bounds, and mutations of the
formulas against the bounds).

TRUTH.  The derivative towers f_0 .. f_5 are written in closed forms without cancellation, so that they keep their relative
accuracy where the header's fp32 forms lose theirs (saturation): tanh through e = exp(-2|z|) (y = sign(z)(1 - e)/(1 + e),
f_1 = sech^2 = 4e/(1 + e)^2), sigmoid through f_1 = s(z) s(-z) and 1 - 2 s = -tanh(z / 2), GELU through Phi = erfc(-z / sqrt 2) / 2.
The jets are `jet_model._dir_fwd` / `_dir_bwd` (checked against autograd in tests/test_jet_model.py) applied to these towers.

BOUNDS.  The argument of tests/term_pde_model.py and tests/term_system_nl_model.py: EPS = 2^-23 bounds one ulp of a value from
above, and a tower entry is a polynomial P_k of an elementary value v that the device function delivers within U ulp:

    bound_k = (U EPS |v| + TINY) |dP_k/dv| + R_k EPS sum|monomials of P_k| + TINY

U is NOT measured on the code under test: it is the single-precision limit of OpenCL 1.2 section 7.4 that
tests/term_system_nl_model.py quotes (tanh 5, exp 3, sin / cos 4, erf 16, x / y 2.5).  R_k counts the fp32 roundings of the
header's expression for f_k (counted from the code, a repeated subexpression counted where it is used; each rounding is half an
EPS, so the count has a factor of two in hand), and the monomials are those of the header's factored expression with every
sign made positive.  TINY = 2^-126 (FLT_MIN) stands for what fp32 cannot resolve below its normal range (expf(100) is inf, so
sigmoid(-100) is 0 and not 3.7e-44).  Where the argument of the elementary function is itself rounded, that is added:

    sin:   |w z| 2^-24 in the argument, i.e. |w z| 2^-24 |cos| on sin and |w z| 2^-24 |sin| on cos
    GELU:  z * z is rounded, so exp(-z^2 / 2) moves by z^2 EPS / 4 of itself; z / sqrt 2 is rounded, so Phi moves by |z| phi EPS / 2
    sigmoid: s = 1 / (1 + expf(-z)) is an exp (3), an addition (0.5) and a division (2.5): U = 6

A jet output is linear in the tower, sum_k f_k m_k(z, ab) with positive integer coefficients in m_k, so

    bound = sum_k bound_k |m_k|(|z|, |ab|) + R EPS sum_k |f_k| |m_k|(|z|, |ab|) + TINY

is the same function evaluated on (bounds, |z|, |ab|) and on (|f|, |z|, |ab|); R = R_FWD, R_BWD, R_MERGED below.
The tape forms evaluate the same polynomials on the fp32 activation value of the forward pass, which is v within U ulp: one
bound serves the direct and the tape form.
"""

from __future__ import annotations

import math
import zlib

import numpy as np
import torch

import jet_model as J

EPS = 2.0 ** -23
TINY = 2.0 ** -126
DENORM = 2.0 ** -149
FLT_MAX = float(np.finfo(np.float32).max)
# OpenCL 1.2, section 7.4, single precision, in ulp (tests/term_system_nl_model.py::U_G)
U_TANH, U_EXP, U_SIN, U_ERF, U_DIV = 5.0, 3.0, 4.0, 16.0, 2.5
U_SIGMOID = U_EXP + 0.5 + U_DIV
# roundings of one jet output: dir_fwd<4>'s last row is 5 summands of at most 5 products and 4 additions; act_bwd's value row
# adds up to 12 summands per direction of at most 6 products each plus the 2 x 12 + 2 additions behind them; merged_bwd's
# value row 4 summands of at most 4 products
R_FWD, R_BWD, R_MERGED = 12, 32, 12
FAMILIES = ("tanh", "sin", "gelu", "sigmoid", "relu")
STREAM_SETS = ((0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (2, 0), (2, 2), (0, 1), (0, 2), (0, 3), (0, 4))
MERGED_CC = (float(np.float32(-0.01 / math.pi)), -1.0)

# the integer coefficient of each order's formula that a mutation changes, and by how much (tests: "the bounds can fail")
COEF = {"tanh": [1, 1, 2, 6, 3, 15], "sin": [1, 1, 1, 1, 1, 1], "gelu": [1, 1, 2, 4, 7, 11], "sigmoid": [1, 1, 2, 6, 12, 12],
        "relu": [1, 1, 0, 0, 0, 0]}
MUTATION = {"tanh": [1, 1, -1, -1, -1, -1], "sin": [1, 1, 1, 1, 1, 1], "gelu": [1, 1, -1, -1, -1, -1],
            "sigmoid": [1, 1, -1, -1, -1, -1], "relu": [1, 1, 1, 1, 1, 1]}
# roundings of the header's expression for f_k
R_TOWER = {"tanh": [0, 2, 3, 6, 7, 9], "sin": [0, 1, 2, 3, 4, 5], "gelu": [2, 4, 3, 4, 6, 7], "sigmoid": [0, 2, 4, 7, 9, 24]}


def f32(v):
    """A Python float that fp32 holds exactly (what a c_float argument becomes)."""
    return float(np.float32(v))


def _t(z):
    return torch.as_tensor(np.asarray(z, dtype=np.float64)) if not isinstance(z, torch.Tensor) else z.double()


def _sigmoid(z):
    e = torch.exp(-z.abs())
    return torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def tower(act, param, z, ord_=5, mutate=None):
    """(f, bound): lists of ord_ + 1 fp64 tensors, f_k(z) and its bound.  act: a family of FAMILIES (leaky_relu and identity
    are "relu" with param 0.01f and 1); param: the fp32 value the kernel gets (sin: w; relu: the slope for z <= 0);
    mutate = k: the integer coefficient COEF[act][k] of f_k changed by MUTATION[act][k]."""
    z = _t(z)
    c = list(COEF[act])
    if mutate is not None:
        c[mutate] += MUTATION[act][mutate]
    w = float(param)
    if act == "tanh":
        e = torch.exp(-2.0 * z.abs())
        y = torch.sign(z) * (1.0 - e) / (1.0 + e)
        f1 = 4.0 * e / (1.0 + e) ** 2
        y2, ya = y * y, y.abs()
        f = [c[0] * y, c[1] * f1, -c[2] * y * f1, f1 * (c[3] * y2 - 2.0), 8.0 * y * f1 * (2.0 - c[4] * y2),
             8.0 * f1 * (2.0 - 15.0 * y2 + c[5] * y2 * y2)]
        dv = U_TANH * EPS * ya + TINY
        dP = [torch.ones_like(y), 2.0 * ya, (6.0 * y2 - 2.0).abs(), (16.0 * y - 24.0 * y * y2).abs(),
              (16.0 - 120.0 * y2 + 120.0 * y2 * y2).abs(), (-272.0 * y + 960.0 * y * y2 - 720.0 * y * y2 * y2).abs()]
        A = [ya, 1.0 + y2, 2.0 * ya * (1.0 + y2), (1.0 + y2) * (6.0 * y2 + 2.0), 8.0 * ya * (1.0 + y2) * (2.0 + 3.0 * y2),
             8.0 * (1.0 + y2) * (2.0 + 15.0 * y2 + 15.0 * y2 * y2)]
        b = [dv * dP[k] + R_TOWER[act][k] * EPS * A[k] + TINY for k in range(6)]
    elif act == "sin":
        x = w * z  # exact in fp64: 24 bits times 24 bits
        s, co = torch.sin(x), torch.cos(x)
        arg = x.abs() * 2.0 ** -24
        ds = U_SIN * EPS * s.abs() + arg * co.abs() + TINY
        dc = U_SIN * EPS * co.abs() + arg * s.abs() + TINY
        sgn = [1.0, 1.0, -1.0, -1.0, 1.0, 1.0]
        f, b = [], []
        for k in range(6):
            v, dvk = (s, ds) if k % 2 == 0 else (co, dc)
            f.append(c[k] * sgn[k] * w ** k * v)
            b.append(abs(w) ** k * dvk + R_TOWER[act][k] * EPS * (abs(w) ** k * v.abs()) + TINY)
    elif act == "gelu":
        z2, za = z * z, z.abs()
        phi = torch.exp(-0.5 * z2) * J.INV_SQRT_2PI
        Phi = 0.5 * torch.erfc(-z * J.SQRT1_2)
        dphi = (U_EXP + 1.0 + 0.25 * z2) * EPS * phi + TINY
        dPhi = 0.5 * U_ERF * EPS * torch.erf(z * J.SQRT1_2).abs() + 0.5 * EPS * za * phi + EPS * Phi + TINY
        Q = [None, None, c[2] - z2, z * (z2 - c[3]), -z2 * z2 + c[4] * z2 - 4.0, z * (z2 * z2 - c[5] * z2 + 18.0)]
        A = [None, None, 2.0 + z2, za * (z2 + 4.0), z2 * z2 + 7.0 * z2 + 4.0, za * (z2 * z2 + 11.0 * z2 + 18.0)]
        f = [c[0] * z * Phi, Phi + c[1] * z * phi] + [phi * Q[k] for k in range(2, 6)]
        b = [za * dPhi + R_TOWER[act][0] * EPS * za * Phi + TINY,
             dPhi + za * dphi + R_TOWER[act][1] * EPS * (Phi + za * phi) + TINY]
        b += [dphi * Q[k].abs() + R_TOWER[act][k] * EPS * phi * A[k] + TINY for k in range(2, 6)]
    elif act == "sigmoid":
        s, sm = _sigmoid(z), _sigmoid(-z)
        g = -torch.tanh(0.5 * z)  # 1 - 2 s
        f1 = s * sm
        f2, f3 = f1 * g, f1 * (1.0 - 6.0 * f1)
        f = [c[0] * s, c[1] * f1, f1 * (g + (2 - c[2]) * s), f1 * (1.0 - c[3] * f1), f2 * (1.0 - c[4] * f1),
             f3 * (1.0 - 12.0 * f1) - c[5] * f2 * f2]
        dv = U_SIGMOID * EPS * s + TINY
        h, q = g * g - 2.0 * f1, 1.0 - 12.0 * f1  # df_2/ds; the factor of f_4 and f_5
        dP = [torch.ones_like(s), g.abs(), h.abs(), (g * q).abs(), (h * q - 12.0 * f2 * g).abs(),
              (g * q * q - 12.0 * g * f3 - 24.0 * f2 * h).abs()]
        A1 = s * (1.0 + s)
        A2, A3 = A1 * (1.0 + 2.0 * s), A1 * (1.0 + 6.0 * A1)
        A = [s, A1, A2, A3, A2 * (1.0 + 12.0 * A1), A3 * (1.0 + 12.0 * A1) + 12.0 * A2 * A2]
        b = [dv * dP[k] + R_TOWER[act][k] * EPS * A[k] + TINY for k in range(6)]
    elif act == "relu":
        m = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, w))
        one = torch.ones_like(z)
        f = [c[0] * z * m, c[1] * m] + [c[k] * one for k in range(2, 6)]
        zero = torch.zeros_like(z)
        b = [EPS * (z * m).abs() + DENORM, zero, zero, zero, zero, zero]
    else:
        raise ValueError(act)
    return f[: ord_ + 1], b[: ord_ + 1]


def _abs(v):
    return [t.abs() for t in v]


def _lin_bound(value_fn, f, b, R):
    """Bound of an output that is linear in the tower: the function on (bounds, |.|) plus R EPS times it on (|f|, |.|)."""
    d, a = value_fn(b), value_fn(_abs(f))
    return [x + R * EPS * y + TINY for x, y in zip(d, a)]


def act_fwd(act, param, z, nt, nx):
    """(a, bound) of act_fwd<ACT, NT, NX> / act_fwd_tape: z = K fp64 tensors in stream order."""
    z = [_t(s) for s in z]
    f, b = tower(act, param, z[0], max(nt, nx, 1))
    za = _abs(z)

    def value(ff, zz):
        return [ff[0]] + J._dir_fwd(ff, zz[1 : 1 + nt]) + J._dir_fwd(ff, zz[1 + nt : 1 + nt + nx])

    a = value(f, z)
    bound = _lin_bound(lambda ff: value(ff, za), f, b, R_FWD)
    bound[0] = b[0]  # the value stream is f_0 itself
    return a, bound


def act_bwd(act, param, z, ab, nt, nx):
    """(zb, bound) of act_bwd<ACT, NT, NX> / act_bwd_tape."""
    z, ab = [_t(s) for s in z], [_t(s) for s in ab]
    f, b = tower(act, param, z[0], max(nt, nx) + 1)
    za, aba = _abs(z), _abs(ab)

    def value(ff, zz, aa):
        ct, zt = J._dir_bwd(ff, zz[1 : 1 + nt], aa[1 : 1 + nt])
        cx, zx = J._dir_bwd(ff, zz[1 + nt : 1 + nt + nx], aa[1 + nt : 1 + nt + nx])
        return [ff[1] * aa[0] + ct + cx] + zt + zx

    zb = value(f, z, ab)
    return zb, _lin_bound(lambda ff: value(ff, za, aba), f, b, R_BWD)


def _merged(f, cc, z, ab):
    """[a_0, a_w, a_x, zb_0, zb_w, zb_x, part] of the merged stream set (jet_device.h: merged_fwd, merged_bwd)."""
    zx2 = z[2] * z[2]
    return [f[0], f[1] * z[1] + cc * f[2] * zx2, f[1] * z[2],
            f[1] * ab[0] + f[2] * z[2] * ab[2] + (f[2] * z[1] + cc * f[3] * zx2) * ab[1],
            f[1] * ab[1], f[1] * ab[2] + 2.0 * cc * f[2] * z[2] * ab[1], ab[1] * f[2] * zx2]


def act_merged(act, param, cc, z, ab):
    """(a, a_bound, zb, zb_bound, part, part_bound) of act_fwd_merged / act_bwd_merged and their tape forms."""
    z, ab = [_t(s) for s in z], [_t(s) for s in ab]
    f, b = tower(act, param, z[0], 3)
    za, aba = _abs(z), _abs(ab)
    v = _merged(f, cc, z, ab)
    bound = _lin_bound(lambda ff: _merged(ff, abs(cc), za, aba), f, b, R_MERGED)
    bound[0] = b[0]
    return v[0:3], bound[0:3], v[3:6], bound[3:6], v[6], bound[6]


def fourier_coef_partial(bx, value):
    bx, value = _t(bx), _t(value)
    p = -(bx * bx) * value
    return p, 2.0 * EPS * p.abs() + TINY


# ---- the inputs of the GPU tests (and of the CPU tests that judge the bounds on them) ------------------------------------------
TOWER_RANGE = {"tanh": 12.0, "sigmoid": 30.0, "gelu": 8.0, "sin": 8.0}
TOWER_EXTRA = {"sigmoid": (100.0, -100.0), "relu": (0.0, -0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX)}
TOWER_PARAMS = {"tanh": (0.0,), "sin": (1.0, 30.0), "gelu": (0.0,), "sigmoid": (0.0,), "relu": (0.0, f32(0.01), 1.0)}
N_TOWER = 1 << 16
N_JET = 4096
JET_SCALES = (1.0, 8.0)  # jets grow like B^k behind Fourier features and SIREN


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _z0(act, n, rng, shrink):
    if act == "relu":
        z = rng.standard_normal(n)
    else:
        R = TOWER_RANGE[act] * shrink
        z = np.concatenate([rng.uniform(-R, R, n // 2), rng.standard_normal(n - n // 2)])
    z = z.astype(np.float32)
    extra = np.asarray(TOWER_EXTRA.get(act, ()), dtype=np.float32)
    z[: extra.size] = extra
    return z


def tower_inputs(act):
    """2^16 fp32 pre-activations: half uniform in [-R, R], half standard normal (relu family: standard normal), the first few
    replaced by the family's extra points."""
    return _z0(act, N_TOWER, _rng("tower", act), 1.0)


def jet_inputs(act, nt, nx, scale, n=N_JET):
    """(z, ab): (K, n) fp32 arrays; z_0 as in `tower_inputs` with R halved, the higher streams standard normal times
    `scale`, the cotangent standard normal."""
    rng = _rng("jet", act, nt, nx, scale)
    K = 1 + nt + nx
    z = (rng.standard_normal((K, n)) * scale).astype(np.float32)
    z[0] = _z0(act, n, rng, 0.5)
    return z, rng.standard_normal((K, n)).astype(np.float32)


def merged_inputs(act, cc, scale, n=N_JET):
    rng = _rng("merged", act, cc, scale)
    z = (rng.standard_normal((3, n)) * scale).astype(np.float32)
    z[0] = _z0(act, n, rng, 0.5)
    return z, rng.standard_normal((3, n)).astype(np.float32)


def ulp_of(v):
    """One ulp of fp32 at the fp64 value v (2^-149 below the normal range)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, TINY)))
    return np.maximum(2.0 ** (e - 23), DENORM)


# ---- an fp32 emulation of the header's expressions (CPU tests only) ------------------------------------------------------------
def _perturb(v64, ulps):
    """fp32 value of v64 moved by `ulps` ulp (non-finite values stay)."""
    v = np.asarray(v64, dtype=np.float64).astype(np.float32)
    with np.errstate(invalid="ignore"):
        moved = (v.astype(np.float64) + ulps * np.spacing(np.abs(v)).astype(np.float64)).astype(np.float32)
    return np.where(np.isfinite(v), moved, v).astype(np.float32)


def emulate_tower(act, param, z, sign):
    """f_0 .. f_5 as the header computes them, in numpy fp32, on an elementary value that is the correctly rounded one moved
    by sign * U / 2 ulp.  The tape form evaluates the same expressions on the same value."""
    z = np.asarray(z, dtype=np.float32)
    z64 = z.astype(np.float64)
    one, w = np.float32(1.0), np.float32(param)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "tanh":
            y = np.clip(_perturb(np.tanh(z64), sign * U_TANH / 2), -one, one)
            y2 = y * y
            f1 = one - y2
            return [y, f1, np.float32(-2.0) * y * f1, f1 * (np.float32(6.0) * y2 - np.float32(2.0)),
                    np.float32(8.0) * y * f1 * (np.float32(2.0) - np.float32(3.0) * y2),
                    np.float32(8.0) * f1 * (np.float32(2.0) - np.float32(15.0) * y2 + np.float32(15.0) * y2 * y2)]
        if act == "sin":
            x = (w * z).astype(np.float64)
            s, c = _perturb(np.sin(x), sign * U_SIN / 2), _perturb(np.cos(x), -sign * U_SIN / 2)
            w2 = w * w
            return [s, w * c, -w2 * s, -w2 * w * c, w2 * w2 * s, w2 * w2 * w * c]
        if act == "gelu":
            z2 = z * z
            phi = _perturb(np.exp((np.float32(-0.5) * z2).astype(np.float64)), sign * U_EXP / 2) * np.float32(0.3989422804014327)
            arg = torch.from_numpy((z * np.float32(0.7071067811865476)).astype(np.float64))
            er = np.clip(_perturb(torch.erf(arg).numpy(), -sign * U_ERF / 2), -one, one)
            Phi = np.float32(0.5) * (one + er)
            return [z * Phi, Phi + z * phi, phi * (np.float32(2.0) - z2), phi * z * (z2 - np.float32(4.0)),
                    phi * (-z2 * z2 + np.float32(7.0) * z2 - np.float32(4.0)),
                    phi * z * (z2 * z2 - np.float32(11.0) * z2 + np.float32(18.0))]
        if act == "sigmoid":
            s = one / (one + _perturb(np.exp(-z64), sign * U_EXP / 2))
            f1 = s * (one - s)
            f2, f3 = f1 * (one - np.float32(2.0) * s), f1 * (one - np.float32(6.0) * f1)
            return [s, f1, f2, f3, f2 * (one - np.float32(12.0) * f1), f3 * (one - np.float32(12.0) * f1) - np.float32(12.0) * f2 * f2]
        m = np.where(z > 0, one, w).astype(np.float32)
        zero = np.zeros_like(z)
        return [z * m, m, zero, zero, zero, zero]


def emulate_jets(act, param, z, ab, nt, nx, sign):
    """(a, zb) of act_fwd / act_bwd in fp32: `jet_model._dir_fwd` / `_dir_bwd` on fp32 tensors and the emulated tower."""
    f = [torch.from_numpy(np.ascontiguousarray(v)) for v in emulate_tower(act, param, z[0], sign)]
    zt = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)) for s in z]
    at = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)) for s in ab]
    a = [f[0]] + J._dir_fwd(f, zt[1 : 1 + nt]) + J._dir_fwd(f, zt[1 + nt : 1 + nt + nx])
    ct, bt = J._dir_bwd(f, zt[1 : 1 + nt], at[1 : 1 + nt])
    cx, bx = J._dir_bwd(f, zt[1 + nt : 1 + nt + nx], at[1 + nt : 1 + nt + nx])
    zb = [f[1] * at[0] + ct + cx] + bt + bx
    assert all(v.dtype == torch.float32 for v in a + zb)
    return a, zb


def emulate_merged(act, param, cc, z, ab, sign):
    f = [torch.from_numpy(np.ascontiguousarray(v)) for v in emulate_tower(act, param, z[0], sign)]
    zt = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)) for s in z]
    at = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)) for s in ab]
    out = _merged(f, float(cc), zt, at)
    assert all(v.dtype == torch.float32 for v in out)
    return out


def worst(err, bound):
    """(worst err / bound, its index) with 0 / 0 = 0 and anything / 0 = inf; NaN counts as inf."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i
