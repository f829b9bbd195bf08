"""GPU: the training-step kernels of csrc/train_kernels.hip, each called directly and compared with the fp64 models of
tests/train_step_model.py: `pinn_jet_losses` and `pinn_point_losses` (loss terms, cotangents, summary4) and
`pinn_adam_clip_step` (sum of squares, clip, Adam).  Every output buffer holds NaN before a call: a slot a kernel leaves
unwritten cannot pass.

Adam starts from theta = 0, so theta is the sum of the updates and rel_l2(theta) measures the update itself (with
theta ~ N(0, 1) and lr = 1e-3 an error of 1e-3 in the update moves theta by 1e-6).  Figures: profiles/train_kernels.md."""

import numpy as np
import pytest
import torch

from conftest import rel_err, rel_l2

import train_step_model as TM

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = np.float32
DELTA = 0.3  # the fp32 number nearest to it is what the kernel and the model get
LOSSES = ["mse", "mae", "huber"]
COUNTS = [1, 255, 256, 257, 1000]  # points per boundary term, around the 256-thread stride
# (cnt / 256 + 8 + 2) * 2^-24 <= 8e-7 for a mean of <= 1000 same-sign fp32 terms through 256 strided partials and an
# eight-level tree; a cotangent is three fp32 operations
LOSS_TOL = 1e-6
MAX_TERMS = 8  # PINN_MAX_POINT_TERMS
RSUM, RSCALE, RW = F32(123.4567), 1.0 / 961.0, 1.7
W_A, W_B, W_PAIR, W_INI = 0.7, 1.3, 0.45, 2.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _stop_at_the_first_gpu_error():
    """A HIP error ends the run of this file: nothing more is launched on a device that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, stopping: {e}", returncode=3)


# ---------------------------------------------------------------------------------------------------------------------
# loss terms
# ---------------------------------------------------------------------------------------------------------------------
def _chain_layout(cnt):
    """The layout of PDEBase._manual_chain with the heat equation's periodic walls, K = 3 streams: two target terms with
    different weights on [0, cnt) of stream 0, one paired term on [0, h) of stream 2 with its partners at [h, 2h), one initial
    term on [cnt, cnt + 100) of stream 0, 37 points no term covers; stream 1 is untouched.  Planted: zero differences (their
    cotangent is exactly 0 under every loss; torch's sign(0) under MAE) and |difference| == delta exactly.
    Returns (jets (3, n) fp32, terms with numpy targets, n_boundary_terms, [(stream, point)] whose cotangent must be 0.0)."""
    rng = np.random.default_rng(4000 + cnt)
    h, n, d = (cnt + 1) // 2, cnt + 137, F32(DELTA)
    J = rng.standard_normal((3, n)).astype(F32)
    tA, tB, tI = (rng.standard_normal(k).astype(F32) for k in (cnt, cnt, 100))
    zeros = []
    for j in (3, 64, 99):
        J[0, cnt + j] = tI[j]
        zeros.append((0, cnt + j))
    tI[7], J[0, cnt + 7] = 0.0, d
    tI[8], J[0, cnt + 8] = d, F32(2.0) * d
    tI[9], J[0, cnt + 9] = 0.0, -d
    if cnt > 4:
        tA[cnt - 1] = tB[cnt - 1] = J[0, cnt - 1]  # both terms of the range tie here
        zeros.append((0, cnt - 1))
        tA[1] = J[0, 1]  # a tie in one of the two terms only
        tA[2], tB[2], J[0, 2] = 0.0, d, F32(2.0) * d  # |r| == delta in both
        J[2, h - 1] = J[2, 2 * h - 1]
        zeros += [(2, h - 1), (2, 2 * h - 1)]
        J[2, 0], J[2, h] = -d, 0.0
    terms = [(0, cnt, 0, 0, tA, W_A), (0, cnt, 0, 0, tB, W_B), (0, h, 2, h, None, W_PAIR), (cnt, cnt + 100, 0, 0, tI, W_INI)]
    return J, terms, 3, zeros


def _eight_term_layout():
    """PINN_MAX_POINT_TERMS terms on (3, 1400) jets: two target terms on one range, paired terms of 257 and 256 points on two
    streams, 255 points on stream 1, an empty term, an initial term and a term on the last point alone."""
    rng = np.random.default_rng(88)
    J = rng.standard_normal((3, 1400)).astype(F32)
    t = lambda k: rng.standard_normal(k).astype(F32)  # noqa: E731
    terms = [(0, 257, 0, 0, t(257), 0.7), (0, 257, 0, 0, t(257), 1.3), (0, 257, 2, 257, None, 0.45), (300, 556, 0, 256, None, 0.8),
             (1000, 1255, 1, 0, t(255), 1.1), (700, 700, 1, 0, t(1), 3.0), (900, 1000, 0, 0, t(100), 2.5), (1399, 1400, 2, 0, t(1), 0.6)]
    return J, terms, 5, [(1, 700), (1, 699), (2, 1398)]


def _dev_terms(terms, dev):
    return [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) if isinstance(x, np.ndarray) else x for x in t) for t in terms]


def _run_losses(dev, J, terms, loss, n_boundary, residual=True, summary=True, point=False):
    """One call with NaN-filled outputs.  point: `point_losses` on the row J (terms (lo, hi, target, weight)).
    Returns (term_losses (9,), cot, summary4 | None) on the host."""
    from pinnrl_amd import engine as E

    jets = torch.from_numpy(J).to(dev)
    dterms = _dev_terms(terms, dev)
    tl = torch.full((MAX_TERMS + 1,), NAN, dtype=torch.float32, device=dev)
    cot = torch.full_like(jets, NAN)
    s4 = torch.full((4,), NAN, dtype=torch.float32, device=dev) if summary else None
    rs = torch.tensor([RSUM], dtype=torch.float32, device=dev) if residual else None
    (E.point_losses if point else E.jet_losses)(jets, dterms, loss, DELTA, tl, cot, rs, RSCALE, RW, n_boundary, s4)
    torch.cuda.synchronize()
    return tl.cpu().numpy(), cot.cpu().numpy(), None if s4 is None else s4.cpu().numpy()


def _check_losses(tag, got, J, terms, loss, n_boundary, zeros, residual=True):
    """`terms` in the jet form.  Losses, cotangent and summary4 against the model at LOSS_TOL; exact zeros where the model's
    cotangent is exactly zero (uncovered points, untouched streams, planted ties)."""
    tl, cot, s4 = got
    cot = cot.reshape(J.shape)
    mterms = [(lo, hi, s, p, tg, TM.r32(w)) for lo, hi, s, p, tg, w in terms]
    L, c64, s64 = TM.jet_loss_terms(J.astype(np.float64), mterms, loss, TM.r32(DELTA), residual_sum=float(RSUM) if residual else None,
                                    residual_scale=TM.r32(RSCALE), residual_weight=TM.r32(RW), n_boundary_terms=n_boundary)
    k = len(terms)
    assert np.isnan(tl[k:]).all(), (tag, "term_losses written past n_terms", tl)
    for i in range(k):
        e = rel_err(tl[i], L[i], label=f"{tag} term {i}", tol=LOSS_TOL)
        print(f"{tag}: term {i} loss {tl[i]:.7e} model {L[i]:.7e} rel err {e:.2e}")
        assert e <= LOSS_TOL, (tag, i, tl[i], L[i])
    covered = np.zeros(J.shape, dtype=bool)
    for lo, hi, s, p, _, _ in terms:
        covered[s, lo:hi] = True
        if p:
            covered[s, lo + p : hi + p] = True
    for s, n in zeros:
        assert c64[s, n] == 0.0, (tag, "the model has a cotangent at a planted zero", s, n)
    assert not c64[~covered].any()
    exact = c64 == 0.0
    assert np.all(cot[exact] == 0.0), (tag, "cotangent where the model has exactly none", np.argwhere(exact & ~(cot == 0.0))[:8])
    if k:
        e = rel_l2(cot, c64, label=f"{tag} cot", tol=LOSS_TOL)
        print(f"{tag}: cot rel l2 {e:.2e}")
        assert e <= LOSS_TOL, (tag, e)
        for s in range(J.shape[0]):
            if c64[s].any():
                e = rel_l2(cot[s], c64[s], label=f"{tag} cot stream {s}", tol=LOSS_TOL)
                assert e <= LOSS_TOL, (tag, s, e)
    else:
        assert np.all(cot == 0.0)
    if s4 is not None:
        for name, a, b in zip(("residual", "boundary", "initial", "total"), s4, s64):
            e = rel_err(a, b, label=f"{tag} summary {name}", tol=LOSS_TOL)
            print(f"{tag}: summary {name} {a:.7e} model {b:.7e} rel err {e:.2e}")
            assert e <= LOSS_TOL, (tag, name, a, b)
    return L, c64, s64


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("loss", LOSSES)
def test_jet_losses_match_the_fp64_model(loss, cnt, dev):
    """The chain layout at every loss kind and count: term losses, cotangent (3 x n) and summary4 against the model at 1e-6;
    the same call again is bit-identical (one workgroup, fixed order); without summary4 and without residual_sum the other
    outputs keep their bits and the summary's residual is 0."""
    J, terms, nb, zeros = _chain_layout(cnt)
    tag = f"jet {loss} cnt={cnt}"
    got = _run_losses(dev, J, terms, loss, nb)
    _check_losses(tag, got, J, terms, loss, nb, zeros)
    assert _same_bits(got, _run_losses(dev, J, terms, loss, nb)), "two calls on the same inputs differ"
    bare = _run_losses(dev, J, terms, loss, nb, summary=False)
    assert bare[2] is None and _same_bits(got[:2], bare[:2])
    nores = _run_losses(dev, J, terms, loss, nb, residual=False)
    assert _same_bits(got[:2], nores[:2])
    _check_losses(tag + " no residual", nores, J, terms, loss, nb, zeros, residual=False)
    assert nores[2][0] == 0.0


@pytest.mark.parametrize("loss", LOSSES)
def test_jet_losses_with_eight_terms_an_empty_term_and_no_terms(loss, dev):
    """n_terms = PINN_MAX_POINT_TERMS (one of them empty: loss exactly 0, no cotangent, where torch's mean would be NaN);
    an empty term first; n_terms = 0: cot all zero, summary4 = {residual, 0, 0, residual_weight * residual}."""
    J, terms, nb, zeros = _eight_term_layout()
    got = _run_losses(dev, J, terms, loss, nb)
    _check_losses(f"jet {loss} eight terms", got, J, terms, loss, nb, zeros)
    assert got[0][5] == 0.0 and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert _same_bits(got, _run_losses(dev, J, terms, loss, nb))

    J2 = J[:, :300].copy()
    two = [(40, 40, 1, 0, np.zeros(1, dtype=F32), 2.0), (0, 257, 0, 0, terms[0][4], 1.5)]
    got = _run_losses(dev, J2, two, loss, 1)
    _, _, s64 = _check_losses(f"jet {loss} empty term", got, J2, two, loss, 1, [(1, 40)])
    assert got[0][0] == 0.0 and got[2][1] == 0.0 and np.all(got[1][1] == 0.0)

    got = _run_losses(dev, J2, [], loss, 0)
    _check_losses(f"jet {loss} no terms", got, J2, [], loss, 0, [])
    assert np.isnan(got[0]).all() and np.all(got[1] == 0.0) and got[2][1] == 0.0 and got[2][2] == 0.0


def _point_cases(cnt):
    """(u, jet-form terms on stream 0, n_boundary, zeros): the K = 1 cases: the target terms of the chain layout, eight target
    terms (one empty), an empty term first, no terms."""
    J, terms, _, zeros = _chain_layout(cnt)
    yield "chain", J[0], [t for t in terms if t[2] == 0 and t[3] == 0], 2, [z for z in zeros if z[0] == 0]
    if cnt == COUNTS[0]:
        rng = np.random.default_rng(99)
        u = rng.standard_normal(1400).astype(F32)
        ranges = [(0, 257), (0, 257), (257, 513), (513, 768), (700, 700), (900, 1000), (0, 1000), (1399, 1400)]
        eight = [(lo, hi, 0, 0, rng.standard_normal(max(hi - lo, 1)).astype(F32), 0.3 + 0.2 * k) for k, (lo, hi) in enumerate(ranges)]
        yield "eight terms", u, eight, 5, [(0, 1398), (0, 1200)]
        yield "empty term", u[:300], [(40, 40, 0, 0, np.zeros(1, dtype=F32), 2.0), eight[0]], 1, [(0, 299)]
        yield "no terms", u[:300], [], 0, []


@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("loss", LOSSES)
def test_point_losses_equal_jet_losses_bit_for_bit_and_match_the_model(loss, cnt, dev):
    """`point_losses` on u equals `jet_losses` on the (1, n) view of u in every bit of term_losses, cot and summary4, and meets
    the model; the eight-term, empty-term and no-term cases ride on the first count."""
    for name, u, terms, nb, zeros in _point_cases(cnt):
        u = np.ascontiguousarray(u)
        pterms = [(lo, hi, tg, w) for lo, hi, _, _, tg, w in terms]
        tag = f"point {loss} cnt={cnt} {name}"
        got = _run_losses(dev, u, pterms, loss, nb, point=True)
        _check_losses(tag, got, u[None, :], terms, loss, nb, zeros)
        as_jets = _run_losses(dev, u[None, :], terms, loss, nb)
        assert _same_bits(got, (as_jets[0], as_jets[1][0], as_jets[2])), tag
        assert _same_bits(got, _run_losses(dev, u, pterms, loss, nb, point=True)), tag
        bare = _run_losses(dev, u, pterms, loss, nb, residual=False, summary=False, point=True)
        assert bare[2] is None and _same_bits(got[:2], bare[:2]), tag
        if name == "empty term":
            assert got[0][0] == 0.0 and got[2][1] == 0.0


def test_bad_terms_are_refused_before_any_launch(dev):
    """Host-side validation: each case raises JetLibraryError and the NaN-filled outputs stay untouched."""
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    K, n = 3, 40
    jets = torch.zeros(K, n, dtype=torch.float32, device=dev)
    tgt = torch.zeros(n, dtype=torch.float32, device=dev)
    ok = (0, 10, 0, 0, tgt, 1.0)
    cases = {
        "hi < lo": [(5, 4, 0, 0, tgt, 1.0)],
        "hi > n_total": [(0, n + 1, 0, 0, tgt, 1.0)],
        "lo < 0": [(-1, 4, 0, 0, tgt, 1.0)],
        "stream < 0": [(0, 10, -1, 0, tgt, 1.0)],
        "stream == K": [(0, 10, K, 0, tgt, 1.0)],
        "paired range overlaps its partner": [(0, 10, 2, 9, None, 1.0)],
        "partner before the range": [(10, 20, 2, -10, None, 1.0)],
        "partner leaves the jets": [(0, 10, 2, n - 9, None, 1.0)],
        "null target of an unpaired term": [(0, 10, 0, 0, None, 1.0)],
        "bad term after a good one": [ok, (0, 10, 2, 5, None, 1.0)],
        "nine terms": [ok] * (MAX_TERMS + 1),
    }
    outs = [torch.full((MAX_TERMS + 1,), NAN, device=dev), torch.full((K, n), NAN, device=dev), torch.full((4,), NAN, device=dev)]
    rs = torch.ones(1, device=dev)
    for name, terms in cases.items():
        with pytest.raises(_lib.JetLibraryError):
            E.jet_losses(jets, terms, "mse", DELTA, outs[0], outs[1], rs, 1.0, 1.0, 1, outs[2])
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs), name
    u, cot1 = jets[0], outs[1][0]
    point_cases = {"hi < lo": [(5, 4, tgt, 1.0)], "hi > n_total": [(0, n + 1, tgt, 1.0)], "lo < 0": [(-1, 4, tgt, 1.0)],
                   "nine terms": [(0, 10, tgt, 1.0)] * (MAX_TERMS + 1)}
    for name, terms in point_cases.items():
        with pytest.raises(_lib.JetLibraryError):
            E.point_losses(u, terms, "mse", DELTA, outs[0], cot1, rs, 1.0, 1.0, 1, outs[2])
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs), name
    E.jet_losses(jets, [ok], "mse", DELTA, outs[0], outs[1], rs, 1.0, 1.0, 1, outs[2])  # and a good call still runs
    torch.cuda.synchronize()
    assert float(outs[0][0]) == 0.0 and bool((outs[1] == 0.0).all()) and float(outs[2][0]) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# clip + Adam
# ---------------------------------------------------------------------------------------------------------------------
# one element; a ragged single sweep (twice); sumsq_kernel's 64 x 256 layout wrapping once plus 3; adam_kernel's 1024-block
# cap plus 37: its grid-stride loop takes a second trip
ADAM_SIZES = [1, 255, 257, 16387, 262181]
# (weight decay, max_norm, gradient scale): no clip; clip active; clip present but inactive; clip active at another bound
SETTINGS = [(0.0, 0.0, 1.0), (1e-2, 1.0, 1.0), (0.0, 1.0, 1e-3), (1e-2, 0.5, 1.0)]
CLIPS = {SETTINGS[0]: None, SETTINGS[1]: True, SETTINGS[2]: False, SETTINGS[3]: True}
NORM_TOL = 1e-6


def _gradient(rng, n, scale):
    """A random direction with |g|_2 = scale * U(3, 6): at least 3x above max_norm = 1 or 0.5 at scale 1, far below at 1e-3,
    at every n (n = 1 included), so that no case sits near the tie norm == max_norm."""
    z = rng.standard_normal(n)
    return (scale * rng.uniform(3.0, 6.0) * z / np.linalg.norm(z)).astype(F32)


class _AdamBuffers:
    """theta = 0, moments, step, lr on the device; `offset` floats off the allocation's alignment.  `grads` is one element longer
    than n and holds 1e6 there (the trainer passes its gradient row with the loss sum stored behind the gradient)."""

    def __init__(self, dev, n, m0=None, v0=None, t0=0, offset=0, lr=1e-3):
        z = lambda k: torch.zeros(k + offset, dtype=torch.float32, device=dev)  # noqa: E731
        self.n, self._raw = n, [z(n), z(n), z(n), z(n + 1)]
        self.theta, self.m, self.v, self.grads = (r[offset:] for r in self._raw)
        if m0 is not None:
            self.m.copy_(torch.from_numpy(m0))
            self.v.copy_(torch.from_numpy(v0))
        self.step = torch.full((1,), float(t0), dtype=torch.float32, device=dev)
        self.lr = torch.full((1,), lr, dtype=torch.float32, device=dev)
        self.scratch = torch.empty(64, dtype=torch.float32, device=dev)
        self.norm = torch.empty(1, dtype=torch.float32, device=dev)

    def run(self, g, wd, max_norm):
        from pinnrl_amd import engine as E

        self.grads[: self.n].copy_(torch.from_numpy(g))
        self.grads[self.n] = 1e6
        self.scratch.fill_(NAN)
        self.norm.fill_(NAN)
        E.adam_clip_step(self.theta, self.grads, self.m, self.v, self.lr, self.step, self.scratch, weight_decay=wd, max_norm=max_norm,
                         grad_norm_out=self.norm)
        torch.cuda.synchronize()


def _compare_adam(tag, n, D, a64, a32, norm, t_want, bad):
    """theta, m, v at max(4 x e32, floor), the norm at 1e-6, the step counter exactly; failures are collected in `bad` so that
    every step's figures are printed."""
    floor = 1e-6 if n == 1 else 3e-7
    if norm is not None:
        e = rel_err(float(D.norm), norm, label=f"{tag} norm", tol=NORM_TOL)
        print(f"{tag}: norm {norm:.6e} device rel err {e:.2e}")
        if not e <= NORM_TOL:
            bad.append((tag, "norm", e, NORM_TOL))
    for name, got, y32, want in (("theta", D.theta, a32.theta, a64.theta), ("m", D.m, a32.m, a64.m), ("v", D.v, a32.v, a64.v)):
        e32 = TM.rel_l2_np(y32, want)
        tol = max(4.0 * e32, floor)
        e = rel_l2(got.cpu(), want, label=f"{tag} {name}", tol=tol)
        print(f"{tag}: {name} device rel l2 {e:.2e} (fp32 restatement {e32:.2e}, tol {tol:.2e})")
        if not e <= tol:
            bad.append((tag, name, e, tol))
    if float(D.step) != t_want:
        bad.append((tag, "step", float(D.step), t_want))


def _adam_sequence(dev, n, wd, max_norm, scale, t0, offset=0, steps=12):
    """`steps` consecutive calls from theta = 0; t0 != 0: the device step counter preset to t0 with moments m != 0, v > 0.
    Returns (failures, [clip active per step], final device buffers)."""
    rng = np.random.default_rng(7 * n + t0 + int(1e4 * wd) + int(10 * max_norm))
    gel = scale * 4.5 / np.sqrt(n)  # a typical gradient element
    m0 = (0.3 * gel * rng.standard_normal(n)).astype(F32) if t0 else None
    v0 = (gel * gel * rng.uniform(0.5, 1.5, n)).astype(F32) if t0 else None
    hp = dict(weight_decay=wd, max_norm=max_norm, m=m0, v=v0, t=t0)
    a64, a32 = TM.make_adam(n, **hp), TM.AdamFp32(n, **hp)
    D = _AdamBuffers(dev, n, m0, v0, t0, offset)
    bad, clipped = [], []
    for s in range(1, steps + 1):
        g = _gradient(rng, n, scale)
        D.run(g, wd, max_norm)
        norm = TM.adam_step(a64, g)
        a32.step(g)
        if max_norm > 0:
            assert norm >= 2.0 * max_norm or norm <= 0.5 * max_norm, "a case must not sit near norm == max_norm"
            clipped.append(norm > max_norm)
        tag = f"adam n={n} wd={wd} max_norm={max_norm} scale={scale} t0={t0} step {s}"
        _compare_adam(tag, n, D, a64, a32, norm, t0 + s, bad)
        if not bool(torch.isfinite(D.scratch).all()):
            bad.append((tag, "scratch64 not fully written"))
        if float(D.grads[n]) != 1e6:
            bad.append((tag, "grads[n] changed"))
    return bad, clipped, D


@pytest.mark.parametrize("wd,max_norm,scale", SETTINGS)
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_clip_step_matches_the_fp64_model(n, wd, max_norm, scale, dev):
    """Twelve steps from step 0 and twelve from step 9 999 (preset moments), theta_0 = 0: theta, m, v, the norm before clipping
    and the step counter after every step against FlatAdam (torch's Adam, bias corrections in double).

    Tolerance per quantity: max(4 x e32, floor), e32 = the error of the specified formulas in numpy fp32 (TM.AdamFp32) on the
    same inputs against FlatAdam; the factor covers fma contraction, rsqrtf / logf / expm1f ulps and the other sum order;
    floor 3e-7 (1e-6 at n = 1: no averaging over elements).  Norm: 1e-6.  `grads[n]` = 1e6 must stay out of the norm.

    Figures (profiles/train_kernels.md), from numpy-fp32 restatements of the kernel on the CPU, n > 1; no device figures
    were taken.  Bias corrections as `1 - powf(beta, t)`: theta of the from-zero sequences 5.6-7.1e-8 at step 1 (powf(b, 1) = b)
    and 6.2e-7-1.6e-6 at steps 2-12, over the tolerance (3.2-5.6e-7) at every one of those steps, 0.6-1.0e-7 from step 9 999.
    As `-expm1f(t * logf(beta))`: theta 0.8-1.4e-7 at every step of both sequences; m <= 1.6e-7, v <= 2.1e-7, norm <= 2.3e-7 in
    either form.  n = 1: theta up to 1.2e-5 (pow) against <= 9.1e-7 (expm1)."""
    failures = []
    for t0 in (0, 9999):
        bad, clipped, _ = _adam_sequence(dev, n, wd, max_norm, scale, t0)
        failures += bad
        want = CLIPS[(wd, max_norm, scale)]
        assert (clipped == []) if want is None else (clipped == [want] * 12), (t0, clipped)
    assert not failures, failures[:6]


def test_adam_clip_step_on_views_off_a_16_byte_boundary(dev):
    """n = 2 with every buffer 4 bytes past a 16-byte boundary (the trainer's coefficient slices): the model's tolerances, and
    the same bits as the aligned run."""
    failures = []
    for t0 in (0, 9999):
        bad, clipped, D = _adam_sequence(dev, 2, 1e-2, 1.0, 1.0, t0, offset=1)
        assert all(b.data_ptr() % 16 == 4 for b in (D.theta, D.m, D.v, D.grads))
        failures += bad
        assert clipped == [True] * 12
        _, _, A = _adam_sequence(dev, 2, 1e-2, 1.0, 1.0, t0, offset=0)
        assert all(torch.equal(a, b) for a, b in ((A.theta, D.theta), (A.m, D.m), (A.v, D.v), (A.norm, D.norm), (A.step, D.step)))
    assert not failures, failures[:6]


def test_graph_of_jet_losses_then_adam_follows_lr_and_new_gradients(dev):
    """[jet_losses -> adam_clip_step] captured as one linear chain on one stream; Adam's gradient buffer is the cotangent
    (3 x 394 parameters).  Three replays, each after new jets and a new learning rate were written into the captured buffers:
    the cotangent follows the loss model, theta, m, v follow FlatAdam on that cotangent with the changed lr, step reads 3."""
    from pinnrl_amd import engine as E

    cnt, loss, wd, max_norm = 257, "mse", 1e-2, 0.1
    J, terms, nb, zeros = _chain_layout(cnt)
    n = J.size
    jets = torch.from_numpy(J).to(dev)
    dterms = _dev_terms(terms, dev)
    tl = torch.empty(MAX_TERMS + 1, dtype=torch.float32, device=dev)
    cot, s4 = torch.empty_like(jets), torch.empty(4, dtype=torch.float32, device=dev)
    rs = torch.tensor([RSUM], dtype=torch.float32, device=dev)
    D = _AdamBuffers(dev, n)

    def launch():
        E.jet_losses(jets, dterms, loss, DELTA, tl, cot, rs, RSCALE, RW, nb, s4)
        E.adam_clip_step(D.theta, cot.view(-1), D.m, D.v, D.lr, D.step, D.scratch, weight_decay=wd, max_norm=max_norm,
                         grad_norm_out=D.norm)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch()  # warm-up outside the capture; its update is discarded below
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for b in (D.theta, D.m, D.v, D.step):
        b.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    torch.cuda.synchronize()
    assert float(D.step) == 0.0 and not bool(D.theta.any()), "capturing must not run the chain"

    a64, a32 = TM.make_adam(n, weight_decay=wd, max_norm=max_norm), TM.AdamFp32(n, weight_decay=wd, max_norm=max_norm)
    rng = np.random.default_rng(17)
    bad = []
    for replay, lr in enumerate((1e-3, 5e-4, 2e-3), start=1):
        Jr = J.copy()
        Jr[:, 10:] += (0.5 * rng.standard_normal(Jr[:, 10:].shape)).astype(F32)  # the planted points beyond 10 move with it
        jets.copy_(torch.from_numpy(Jr))
        D.lr.fill_(lr)
        for b in (tl, cot, s4, D.scratch, D.norm):
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        tag = f"graph replay {replay}"
        _check_losses(tag, (tl.cpu().numpy(), cot.cpu().numpy(), s4.cpu().numpy()), Jr, terms, loss, nb, [])
        g = cot.cpu().numpy().ravel()
        a64.lr, a32.lr = TM.r32(lr), F32(lr)
        norm = TM.adam_step(a64, g)
        a32.step(g)
        assert norm >= 2.0 * max_norm, norm
        _compare_adam(tag, n, D, a64, a32, norm, replay, bad)
    assert not bad, bad[:6]
    assert float(D.step) == 3.0
