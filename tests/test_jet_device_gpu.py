"""The HIP text of csrc/jet_device.h, element by element, against fp64 (tests/jet_device_model.py) through the probe library
(tests/probe/jet_device_probe.hip -> libpinnjet_probe.so, tests/jet_device_probe.py).

(a), (b): the two hand-written elementary functions against double over all of fp32 (a strided sweep plus the places where they
switch branch), with the device library's own functions on the same inputs as a control.  (c): the derivative towers, orders 1
and 5, direct and tape form, each row within the model's condition-aware bound.  (d): act_fwd / act_bwd and their tape forms on
the twelve compiled stream sets.  (e): the merged forms.  The bars of (a) and (b) and the bounds of the model are set by
reasoning (the model's docstring), not from what these tests measure; the measurements are in profiles/jet_device_accuracy.md.
No point is skipped: fp32 inputs are exact, the relu kink included.
"""

import math

import numpy as np
import pytest
import torch

import jet_device_model as M
import jet_device_probe as P

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -24  # the unit of the absolute bar of fast_sincosf: one ulp of a value in [0.5, 1)
PI_4 = math.pi / 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    P.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _stop_at_the_first_gpu_error():
    """A HIP error ends the run of this file: nothing more is launched on a device that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, stopping: {e}", returncode=3)


def _bits(lo, hi, step=1):
    return np.arange(lo, hi, step, dtype=np.int64).astype(np.uint32).view(np.float32)


def _both_signs(x):
    return np.concatenate([x, -x])


def _strided_sweep():
    """Every 2^11-th bit pattern of the finite floats, both signs."""
    return _both_signs(_bits(0, 0x7F800000, 1 << 11))


def _around(c, ulps=4096):
    b = int(np.float32(c).view(np.uint32))
    return _both_signs(_bits(max(b - ulps, 0), b + ulps + 1))


def _alternate(x):
    x = np.asarray(x, dtype=np.float32).copy()
    x[1::2] *= -1.0
    return x


def _run_chunks(fn, x, dev):
    """fn on x in launches of at most P.MAX_LAUNCH elements; the outputs as fp64 numpy arrays."""
    outs = None
    for lo in range(0, x.size, P.MAX_LAUNCH):
        got = fn(torch.from_numpy(x[lo : lo + P.MAX_LAUNCH]).to(dev))
        torch.cuda.synchronize()
        got = [g.cpu().numpy() for g in got]
        outs = [[g] for g in got] if outs is None else [o + [g] for o, g in zip(outs, got)]
    return [np.concatenate(o) for o in outs]


def _worst(err, x):
    i = int(np.argmax(err))
    return float(err[i]), float(x[i])


def test_fast_sincosf(dev):
    """(a) Bars against fp64: |x| <= pi/4: 4 ulp of the true value; pi/4 < |x| <= 8192: 4 x 2^-24 absolute (near the zeros the
    error in ulps of the result is unbounded: a host transcription measures 1.56 x 2^-24 and 688 ulp); above, the library path:
    4 ulp."""
    rng = np.random.default_rng(71)
    k = np.arange(1, 5216)
    near = (np.float32(k * (math.pi / 2)).view(np.uint32).astype(np.int64)[:, None] + np.arange(-3, 4)[None, :]).astype(np.uint32)
    parts = [_strided_sweep(), _around(0.0), _around(PI_4), _around(8192.0), _alternate(near.view(np.float32).reshape(-1))]
    for lo, hi in ((0.0, PI_4), (PI_4, 64.0), (64.0, 1024.0), (1024.0, 8192.0)):
        parts.append(_alternate(rng.uniform(lo, hi, 1 << 20)))
    x = np.concatenate(parts).astype(np.float32)
    assert np.isfinite(x).all()
    s, c, s_lib, c_lib = _run_chunks(P.sincos, x, dev)
    x64 = x.astype(np.float64)
    ts, tc = np.sin(x64), np.cos(x64)
    ax = np.abs(x64)
    regions = (("|x| <= pi/4", ax <= PI_4, "ulp"), ("pi/4 < |x| <= 8192", (ax > PI_4) & (ax <= 8192.0), "abs"),
               ("|x| > 8192 (library path)", ax > 8192.0, "ulp"))
    assert sum(int(m.sum()) for _, m, _ in regions) == x.size
    failures = []
    for name, mask, unit in regions:
        for fn, got, lib, truth in (("sin", s, s_lib, ts), ("cos", c, c_lib, tc)):
            g, l, t, xs = got[mask], lib[mask], truth[mask], x64[mask]
            assert np.isfinite(g).all(), (name, fn)
            e_abs, e_ulp = np.abs(g - t) / ULP1, np.abs(g - t) / M.ulp_of(t)
            l_abs, l_ulp = np.abs(l - t) / ULP1, np.abs(l - t) / M.ulp_of(t)
            (wa, xa), (wu, xu) = _worst(e_abs, xs), _worst(e_ulp, xs)
            print(f"fast_sincosf {fn} {name} ({int(mask.sum())} points): worst {wa:.3f} x 2^-24 at x = {xa!r}, {wu:.3f} ulp of the true "
                  f"value at x = {xu!r}; library {fn}f {l_abs.max():.3f} x 2^-24, {l_ulp.max():.3f} ulp; bar 4 ({unit})")
            if (wa if unit == "abs" else wu) > 4.0:
                failures.append((fn, name, wa, wu))
    nan = torch.tensor([float("nan"), -float("nan")], dtype=torch.float32, device=dev)
    for out in P.sincos(nan)[:2]:
        assert torch.isnan(out).all()
    z = P.sincos(torch.tensor([-0.0, 0.0], dtype=torch.float32, device=dev))
    print(f"fast_sincosf sin(-0.0f) = {'-' if bool(torch.signbit(z[0][0])) else '+'}0 (library sinf: "
          f"{'-' if bool(torch.signbit(z[2][0])) else '+'}0)")
    assert not failures, failures


def test_fast_tanhf(dev):
    """(b) 5 ulp of the true value for every finite z; |y| <= 1 always; tanh(+-0) = +-0; +-inf -> +-1; NaN -> NaN."""
    denorm = _both_signs(np.concatenate([_bits(1, 65), _bits(0x007FFFC0, 0x00800000)]))
    finite = np.concatenate([_strided_sweep(), _around(0.625), _alternate(np.linspace(8.9, 9.2, 1 << 16)), denorm,
                             np.asarray([0.0, -0.0], dtype=np.float32)]).astype(np.float32)
    special = np.asarray([np.inf, -np.inf, np.nan], dtype=np.float32)
    z = np.concatenate([finite, special])
    y, y_lib = _run_chunks(P.tanh, z, dev)
    nf = finite.size
    z64 = finite.astype(np.float64)
    t = np.tanh(z64)
    e, e_lib = np.abs(y[:nf] - t) / M.ulp_of(t), np.abs(y_lib[:nf] - t) / M.ulp_of(t)
    worst = 0.0
    for name, mask in (("|z| < 0.625 (polynomial)", np.abs(z64) < 0.625), ("|z| >= 0.625 (exp2 / rcp)", np.abs(z64) >= 0.625)):
        w, zw = _worst(e[mask], z64[mask])
        worst = max(worst, w)
        print(f"fast_tanhf {name} ({int(mask.sum())} points): worst {w:.3f} ulp of the true value at z = {zw!r}; library tanhf "
              f"{e_lib[mask].max():.3f} ulp; bar 5")
    assert np.isfinite(y[:nf]).all()
    assert (np.abs(y[: nf + 2]) <= 1.0).all(), "1 - y * y must never be negative"
    zero = finite == 0.0
    assert zero.sum() >= 2 and (y[:nf][zero] == 0.0).all() and (np.signbit(y[:nf][zero]) == np.signbit(finite[zero])).all()
    assert y[nf] == 1.0 and y[nf + 1] == -1.0 and np.isnan(y[nf + 2])
    assert worst <= 5.0, worst


def _check_rows(label, got, want, bound, z0, failures):
    """Every row of got (K, n) within its bound; prints the worst error / bound of the case and where it occurred."""
    got = got.cpu().numpy().astype(np.float64)
    worst = (0.0, 0, 0)
    for s in range(got.shape[0]):
        r, i = M.worst(np.abs(got[s] - want[s].numpy()), bound[s].numpy())
        if not np.isfinite(got[s]).all():
            r, i = np.inf, int(np.argmin(np.isfinite(got[s])))
        if r >= worst[0]:
            worst = (r, s, i)
    print(f"{label}: worst error / bound {worst[0]:.3f} in row {worst[1]} at z_0 = {float(z0[worst[2]])!r}")
    if not worst[0] <= 1.0:
        failures.append((label, worst))
    return worst[0]


@pytest.mark.parametrize("act", M.FAMILIES)
def test_derivative_towers(dev, act):
    """(c) act_derivs / act_derivs_tape, orders 1 and 5: every row within its bound on 2^16 points per parameter; the
    piecewise-linear family bit for bit; no output that is not finite where the family promises one."""
    z = M.tower_inputs(act)
    zt = torch.from_numpy(z).to(dev)
    failures = []
    for w in M.TOWER_PARAMS[act]:
        f, b = M.tower(act, w, z)
        for ord_ in (1, 5):
            for tape in (0, 1):
                got = P.act_derivs(act, ord_, w, tape, zt)
                _check_rows(f"act_derivs {act} param {w:g} order {ord_} {'tape' if tape else 'direct'}", got, f, b, z, failures)
                if act == "relu":
                    m = np.where(z > 0, np.float32(1.0), np.float32(w)).astype(np.float32)
                    want = [z * m, m] + [np.zeros_like(z)] * 4
                    for k in range(ord_ + 1):
                        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), (w, ord_, tape, k)
    if act in ("tanh", "sigmoid"):
        wide = np.concatenate([_strided_sweep(), np.asarray([np.inf, -np.inf], dtype=np.float32)])
    elif act in ("gelu", "sin"):
        wide = np.concatenate([np.linspace(-1e4, 1e4, 1 << 16), [1e4, -1e4]]).astype(np.float32)
    else:
        wide = None
    if wide is not None:
        for w in M.TOWER_PARAMS[act]:
            for tape in (0, 1):
                for lo in range(0, wide.size, P.MAX_LAUNCH):
                    got = P.act_derivs(act, 5, w, tape, torch.from_numpy(wide[lo : lo + P.MAX_LAUNCH]).to(dev))
                    assert bool(torch.isfinite(got).all()), (act, w, tape)
    assert not failures, failures


def _leaky_names(act, w):
    """The activation ids a parameter of the piecewise-linear family is reached through (all take the relu branch)."""
    if act != "relu":
        return (act,)
    return {0.0: ("relu",), M.f32(0.01): ("leaky_relu",), 1.0: ("identity",)}[w]


@pytest.mark.parametrize("act", M.FAMILIES)
def test_act_fwd_bwd(dev, act):
    """(d) act_fwd, act_bwd and the tape forms on the twelve stream sets, 4096 points, higher streams at scale 1 and 8: every row
    within its propagated bound; direct and tape form each against fp64, not against each other."""
    failures = []
    for w in M.TOWER_PARAMS[act]:
        for name in _leaky_names(act, w):
            for scale in M.JET_SCALES:
                for nt, nx in M.STREAM_SETS:
                    z, ab = M.jet_inputs(act, nt, nx, scale)
                    a, a_b = M.act_fwd(act, w, z, nt, nx)
                    zb, zb_b = M.act_bwd(act, w, z, ab, nt, nx)
                    zt, abt = torch.from_numpy(z).to(dev), torch.from_numpy(ab).to(dev)
                    for tape in (0, 1):
                        tag = f"{name} param {w:g} ({nt},{nx}) x{scale:g} {'tape' if tape else 'direct'}"
                        _check_rows(f"act_fwd {tag}", P.act_fwd(name, nt, nx, w, tape, zt), a, a_b, z[0], failures)
                        _check_rows(f"act_bwd {tag}", P.act_bwd(name, nt, nx, w, tape, zt, abt), zb, zb_b, z[0], failures)
    assert not failures, failures


@pytest.mark.parametrize("act", M.FAMILIES)
def test_merged_forms(dev, act):
    """(e) act_fwd_merged, act_bwd_merged, their tape variants and the coefficient partial, c in {-0.01 / pi, -1}."""
    failures = []
    for w in M.TOWER_PARAMS[act]:
        for name in _leaky_names(act, w):
            for scale in M.JET_SCALES:
                for cc in M.MERGED_CC:
                    z, ab = M.merged_inputs(act, cc, scale)
                    a, a_b, zb, zb_b, part, part_b = M.act_merged(act, w, cc, z, ab)
                    zt, abt = torch.from_numpy(z).to(dev), torch.from_numpy(ab).to(dev)
                    for tape in (0, 1):
                        ga, gzb, gp = P.act_merged(name, w, cc, tape, zt, abt)
                        tag = f"{name} param {w:g} c = {cc:.6g} x{scale:g} {'tape' if tape else 'direct'}"
                        _check_rows(f"act_fwd_merged {tag}", ga, a, a_b, z[0], failures)
                        _check_rows(f"act_bwd_merged {tag}", gzb, zb, zb_b, z[0], failures)
                        _check_rows(f"coefficient partial {tag}", gp[None], [part], [part_b], z[0], failures)
    assert not failures, failures


def test_fourier_coef_partial_merged(dev):
    rng = np.random.default_rng(73)
    bx = (rng.standard_normal(M.N_JET) * 8.0).astype(np.float32)
    value = rng.uniform(-1.0, 1.0, M.N_JET).astype(np.float32)
    got = P.fourier_coef_partial(torch.from_numpy(bx).to(dev), torch.from_numpy(value).to(dev))
    want, bound = M.fourier_coef_partial(bx, value)
    failures = []
    _check_rows("fourier_coef_partial_merged", got[None], [want], [bound], bx, failures)
    assert not failures, failures
