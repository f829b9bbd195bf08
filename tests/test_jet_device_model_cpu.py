"""tests/jet_device_model.py judged on the CPU, before tests/test_jet_device_gpu.py holds the HIP text of csrc/jet_device.h to it:

  * the cancellation-free closed forms against mpmath at 50 digits (1e-13 relative, |z| = 20 included), and against the models
    that are already checked against autograd (tests/jet_model.py, tests/merged_model.py);
  * an fp32 emulation of the header's expressions, on an elementary value moved by U / 2 ulp either way, stays inside every bound
    on the inputs of the GPU tests: the bounds are not too tight for what the number format alone does;
  * a formula with one integer coefficient changed by one leaves twice its bound at no less than half of those inputs: the bounds
    are not so loose that a wrong coefficient would pass.
"""

import mpmath
import numpy as np
import pytest
import torch

import jet_device_model as M
import jet_model as J
import merged_model as MM

ACT_NAME = {0.0: "relu", M.f32(0.01): "leaky_relu", 1.0: "identity"}


def _mp_function(act, w):
    mp = mpmath.mp
    if act == "tanh":
        return mp.tanh
    if act == "sin":
        return lambda x: mp.sin(w * x)
    if act == "gelu":
        return lambda x: x * mp.erfc(-x / mp.sqrt(2)) / 2
    assert act == "sigmoid"
    return lambda x: 1 / (1 + mp.exp(-x))


def _mp_gelu(x):
    """Derivatives 0 .. 5 of x Phi(x) by Leibniz and phi^(n) = (-1)^n He_n phi (He by its recurrence): numerical differentiation
    at 50 digits cannot resolve values of 1e-89, which GELU has at x = -20."""
    mp = mpmath.mp
    phi = mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)
    he = [mpmath.mpf(1), x]
    for n in range(1, 5):
        he.append(x * he[n] - n * he[n - 1])
    dphi = [(-1) ** n * he[n] * phi for n in range(5)]  # phi^(n); Phi^(k) = phi^(k-1)
    Phi = mp.erfc(-x / mp.sqrt(2)) / 2
    return [x * Phi, Phi + x * phi] + [k * dphi[k - 2] + x * dphi[k - 1] for k in range(2, 6)]


@pytest.mark.parametrize("act", M.FAMILIES)
def test_closed_forms_against_mpmath(act):
    """f_0 .. f_5 of the model against the Taylor coefficients mpmath computes at 50 digits, 288 points in [-20, 20] per parameter
    (288 and not 300: a point of the 300-grid lies 3e-3 from a zero of sigmoid's f_5, where the relative difference of any fp64
    formula is the conditioning of the zero, 4e-13 there, and says nothing about the closed form)."""
    z = np.linspace(-20.0, 20.0, 288).astype(np.float32)
    assert abs(z[0]) == 20.0 and abs(z[-1]) == 20.0
    worst = (0.0, None)
    with mpmath.workdps(50):
        for w in M.TOWER_PARAMS[act]:
            f, _ = M.tower(act, w, z)
            f = [v.numpy() for v in f]
            for i, zi in enumerate(z):
                x = mpmath.mpf(float(zi))
                if act == "relu":
                    m = mpmath.mpf(1) if zi > 0 else mpmath.mpf(w)
                    want = [x * m, m, 0, 0, 0, 0]
                elif act == "gelu":
                    want = _mp_gelu(x)
                else:
                    co = mpmath.taylor(_mp_function(act, mpmath.mpf(w)), x, 5)
                    want = [co[k] * mpmath.factorial(k) for k in range(6)]
                for k in range(6):
                    err = abs(mpmath.mpf(float(f[k][i])) - want[k])
                    rel = float(err / abs(want[k])) if want[k] != 0 else (0.0 if err == 0 else np.inf)
                    if rel > worst[0]:
                        worst = (rel, (w, k, float(zi)))
    print(f"{act}: worst relative difference to mpmath {worst[0]:.2e} at (param, order, z) = {worst[1]}")
    assert worst[0] <= 1e-13


@pytest.mark.parametrize("act", M.FAMILIES)
def test_model_agrees_with_the_autograd_checked_models(act):
    """Where nothing saturates the closed forms are the formulas of jet_model.py / merged_model.py: towers, jets, adjoints, merged."""
    rng = np.random.default_rng(5)
    n = 512
    for w in M.TOWER_PARAMS[act]:
        name = ACT_NAME[w] if act == "relu" else act
        if name == "leaky_relu":
            w = 0.01  # jet_model's slope is the fp64 number, not the fp32 one the kernels get
        for nt, nx in M.STREAM_SETS:
            K = 1 + nt + nx
            z = [torch.from_numpy(rng.uniform(-2.5, 2.5, n) if s == 0 else rng.standard_normal(n)) for s in range(K)]
            ab = [torch.from_numpy(rng.standard_normal(n)) for _ in range(K)]
            a, _ = M.act_fwd(act, w, z, nt, nx)
            zb, _ = M.act_bwd(act, w, z, ab, nt, nx)
            for got, want in zip(a + zb, J.act_fwd(name, w, z, nt, nx) + J.act_bwd(name, w, z, ab, nt, nx)):
                assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))
        z = [torch.from_numpy(rng.uniform(-2.5, 2.5, n))] + [torch.from_numpy(rng.standard_normal(n)) for _ in range(2)]
        ab = [torch.from_numpy(rng.standard_normal(n)) for _ in range(3)]
        for cc in M.MERGED_CC:
            a, _, zb, _, part, _ = M.act_merged(act, w, cc, z, ab)
            zb_want, part_want = MM.act_bwd(name, w, cc, z, ab)
            for got, want in zip(a + zb + [part], MM.act_fwd(name, w, cc, z) + zb_want + [part_want]):
                assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))


def _inside(label, got, want, bound, worst_of):
    for s, (g, t, b) in enumerate(zip(got, want, bound)):
        g = np.asarray(g, dtype=np.float64)
        assert np.isfinite(g).all(), (label, s)
        r, i = M.worst(np.abs(g - t.numpy()), b.numpy())
        worst_of[0] = max(worst_of[0], r)
        assert r <= 1.0, f"{label} row {s}: emulation at {r:.3f} of the bound, element {i}"


@pytest.mark.parametrize("act", M.FAMILIES)
def test_fp32_emulation_stays_inside_the_bounds(act):
    worst_of = [0.0]
    for w in M.TOWER_PARAMS[act]:
        z = M.tower_inputs(act)
        f, b = M.tower(act, w, z)
        for sign in (1.0, -1.0):
            _inside(f"tower {act} {w} {sign:+.0f}", M.emulate_tower(act, w, z, sign), f, b, worst_of)
        for scale in M.JET_SCALES:
            for nt, nx in M.STREAM_SETS:
                z, ab = M.jet_inputs(act, nt, nx, scale)
                a, a_b = M.act_fwd(act, w, z, nt, nx)
                zb, zb_b = M.act_bwd(act, w, z, ab, nt, nx)
                for sign in (1.0, -1.0):
                    ea, ezb = M.emulate_jets(act, w, z, ab, nt, nx, sign)
                    _inside(f"act_fwd {act} {w} ({nt},{nx}) x{scale} {sign:+.0f}", [v.numpy() for v in ea], a, a_b, worst_of)
                    _inside(f"act_bwd {act} {w} ({nt},{nx}) x{scale} {sign:+.0f}", [v.numpy() for v in ezb], zb, zb_b, worst_of)
            for cc in M.MERGED_CC:
                z, ab = M.merged_inputs(act, cc, scale)
                a, a_b, zb, zb_b, part, part_b = M.act_merged(act, w, cc, z, ab)
                for sign in (1.0, -1.0):
                    em = M.emulate_merged(act, w, cc, z, ab, sign)
                    _inside(f"merged {act} {w} c={cc} x{scale} {sign:+.0f}", [v.numpy() for v in em], a + zb + [part],
                            a_b + zb_b + [part_b], worst_of)
    print(f"{act}: the fp32 emulation reaches {worst_of[0]:.3f} of a bound at the most")


@pytest.mark.parametrize("act", M.FAMILIES)
def test_a_wrong_tower_coefficient_leaves_the_bounds(act):
    """Per order: one integer coefficient of the model's formula changed by one (tanh: 6 -> 5 in f_3, 3 -> 2 in f_4, 15 -> 14 in f_5)
    differs from the truth by more than twice the bound at no less than half of the family's GPU input points (all its parameters)."""
    z = M.tower_inputs(act)
    for k in range(6):
        hit = total = 0
        for w in M.TOWER_PARAMS[act]:
            f, b = M.tower(act, w, z)
            g, _ = M.tower(act, w, z, mutate=k)
            hit += int(((g[k] - f[k]).abs() > 2.0 * b[k]).sum())
            total += z.size
        print(f"{act} f_{k}: coefficient {M.COEF[act][k]} -> {M.COEF[act][k] + M.MUTATION[act][k]} leaves twice the bound at "
              f"{100.0 * hit / total:.1f} % of the points")
        assert hit >= 0.5 * total, (act, k, hit / total)


@pytest.mark.parametrize("act", [a for a in M.FAMILIES if a != "relu"])  # relu: f_3 = 0, the changed monomials vanish
def test_a_wrong_jet_coefficient_leaves_the_bounds(act):
    """dir_fwd<4>: 6 -> 5 in 6 f_3 z_1^2 z_2 of the fourth row; dir_bwd<4>: 12 -> 11 in 12 f_3 z_1 z_2 ab_4 of zb_1.  The change of
    the output is the monomial itself; it must exceed twice the row's bound at no less than half of the points of the sets that
    reach order 4."""
    for which in ("dir_fwd", "dir_bwd"):
        hit = total = 0
        for w in M.TOWER_PARAMS[act]:
            for scale in M.JET_SCALES:
                for nt, nx in ((1, 4), (0, 4)):
                    z, ab = M.jet_inputs(act, nt, nx, scale)
                    zt, at = [torch.from_numpy(s).double() for s in z], [torch.from_numpy(s).double() for s in ab]
                    f, _ = M.tower(act, w, zt[0], 5)
                    x = zt[1 + nt :]
                    if which == "dir_fwd":
                        _, bound = M.act_fwd(act, w, z, nt, nx)
                        change, row = f[3] * x[0] ** 2 * x[1], nt + 4
                    else:
                        _, bound = M.act_bwd(act, w, z, ab, nt, nx)
                        change, row = f[3] * x[0] * x[1] * at[nt + 4], nt + 1
                    hit += int((change.abs() > 2.0 * bound[row]).sum())
                    total += change.numel()
        print(f"{act} {which}<4>: the changed coefficient leaves twice the bound at {100.0 * hit / total:.1f} % of the points")
        assert hit >= 0.5 * total, (act, which, hit / total)


def test_the_jet_mutation_is_the_stated_monomial():
    """The two monomials above are what the coefficient multiplies in jet_model._dir_fwd / _dir_bwd (their derivative with
    respect to the coefficient), checked by differencing the model with f_3 switched on and off."""
    rng = np.random.default_rng(9)
    z = [torch.from_numpy(rng.standard_normal(64)) for _ in range(4)]
    ab = [torch.from_numpy(rng.standard_normal(64)) for _ in range(4)]
    zero = torch.zeros(64, dtype=torch.float64)
    f3 = torch.from_numpy(rng.standard_normal(64))
    only_f3 = [zero, zero, zero, f3, zero, zero]
    y = J._dir_fwd(only_f3, z)
    assert torch.allclose(y[3], 6.0 * f3 * z[0] ** 2 * z[1], rtol=1e-14, atol=0)
    _, zb = J._dir_bwd(only_f3, z, [zero, zero, zero, ab[3]])
    assert torch.allclose(zb[0], 12.0 * f3 * z[0] * z[1] * ab[3], rtol=1e-14, atol=0)
