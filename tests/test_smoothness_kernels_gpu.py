"""GPU: `pinn_fd_stencil_points` and `pinn_fd_smoothness` (csrc/train_kernels.hip) against the models of
tests/smoothness_model.py.

Sizes: 1 (a single point), 37 (segment bases at N and 2N not 16-byte aligned, a partial last quad), 1000 (an exact multiple:
every segment takes 16-byte accesses), 1027 (several workgroups, misaligned bases, a partial last quad).  Every batch larger
than one point holds points exactly on either domain end (the clamp ties them to their shifted copies), points within eps/2
of either end (clamp active, no tie) and interior points."""

import numpy as np
import pytest
import torch

import smoothness_model as SM

pytestmark = pytest.mark.gpu

SIZES = (1, 37, 1000, 1027)
EPSS = (1e-4, 2.0**-6)
LO, HI = 0.0, 2.0
U = 2.0**-23  # spacing of fp32 at 1: bounds below are multiples of it, relative


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _E():
    import pinnrl_amd  # noqa: F401
    from pinnrl_amd import engine

    return engine


def _batch(n, eps, seed=0):
    rng = np.random.default_rng(seed + n)
    x = (LO + (HI - LO) * rng.random(n)).astype(np.float32)
    t = (10.0 * rng.random(n)).astype(np.float32)
    if n == 1:
        x[0] = HI
    else:
        idx = rng.permutation(n)
        k = max(n // 12, 1)
        x[idx[:k]] = LO
        x[idx[k : 2 * k]] = HI
        x[idx[2 * k : 3 * k]] = np.float32(LO + 0.5 * eps * rng.random(k))
        x[idx[3 * k : 4 * k]] = np.float32(HI - 0.5 * eps * rng.random(k))
    return x, t


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("n", SIZES)
def test_stencil_points_equal_torch_bit_for_bit(n, eps, dev):
    E = _E()
    xh, th = _batch(n, eps)
    for offset in (0, 1):  # offset 1: the inputs themselves are not 16-byte aligned
        xb, tb = torch.zeros(n + 1, device=dev), torch.zeros(n + 1, device=dev)
        x, t = xb[offset : offset + n], tb[offset : offset + n]
        x.copy_(torch.from_numpy(xh))
        t.copy_(torch.from_numpy(th))
        x3 = torch.full((3 * n + 8,), -7.0, device=dev)
        t3 = torch.full((3 * n + 8,), -7.0, device=dev)
        E.fd_stencil_points(x, t, eps, LO, HI, x3[: 3 * n], t3[: 3 * n])
        want = torch.cat([x, torch.clamp(x + eps, LO, HI), torch.clamp(x - eps, LO, HI)])
        assert torch.equal(x3[: 3 * n], want), (n, eps, offset)
        assert torch.equal(t3[: 3 * n], torch.cat([t, t, t]))
        assert bool((x3[3 * n :] == -7.0).all()) and bool((t3[3 * n :] == -7.0).all())  # nothing past the 3N floats
        mx, mt = SM.stencil_points(xh, th, eps, LO, HI)
        assert np.array_equal(x3[: 3 * n].cpu().numpy(), mx) and np.array_equal(t3[: 3 * n].cpu().numpy(), mt)
    if n > 1:
        xc, xp, xm = want[:n], want[n : 2 * n], want[2 * n :]
        assert bool((xp == xc).any()) and bool((xm == xc).any())  # ties at the ends
        assert bool(((xp == HI) & (xc < HI)).any()) and bool(((xm == LO) & (xc > LO)).any())  # clamp active without a tie


def _values(n, seed=1):
    """A synthetic [uc | up | um]: differences of both signs and of very different sizes, planted exact ties."""
    rng = np.random.default_rng(seed + n)
    uc = rng.standard_normal(n).astype(np.float32)
    up = (uc + (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -1, n)).astype(np.float32)).astype(np.float32)
    um = (uc + (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -1, n)).astype(np.float32)).astype(np.float32)
    if n == 1:
        up[0] = uc[0]
    else:
        idx = rng.permutation(n)
        k = max(n // 10, 1)
        up[idx[:k]] = uc[idx[:k]]
        um[idx[k : 2 * k]] = uc[idx[k : 2 * k]]
        um[idx[2 * k]], up[idx[2 * k]] = uc[idx[2 * k]], uc[idx[2 * k]]  # both at once
    return np.concatenate([uc, up, um])


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("n", SIZES)
def test_smoothness_against_the_fp64_model(n, eps, dev):
    E = _E()
    from pinnrl_amd import _lib

    u3h = _values(n)
    weight = 0.1
    w32 = float(np.float32(weight))  # the number the fp32 argument carries
    S, cot = SM.smoothness_terms(u3h, eps, w32)
    u3 = torch.from_numpy(u3h).to(dev)
    scratch = torch.zeros(_lib.PINN_FD_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    runs = []
    for before in (0.0, 0.0, 0.625):
        loss = torch.full((1,), -7.0, device=dev)
        cot3 = torch.full((3 * n + 8,), -7.0, device=dev)
        summary = torch.tensor([1.0, 2.0, 3.0, before], device=dev)
        E.fd_smoothness(u3, eps, weight, loss, cot3[: 3 * n], scratch, summary4=summary)
        assert bool((cot3[3 * n :] == -7.0).all())
        runs.append((loss.cpu().numpy().copy(), cot3[: 3 * n].cpu().numpy().copy(), summary.cpu().numpy().astype(np.float64)))
    (l0, c0, s0), (l1, c1, s1), (l2, c2, s2) = runs
    assert l0.tobytes() == l1.tobytes() and c0.tobytes() == c1.tobytes() and s0.tobytes() == s1.tobytes()  # bit-identical
    e_S = abs(float(l0[0]) - S) / S
    print(f"N {n} eps {eps:.3e}: S {float(l0[0])!r} vs {S!r}: rel {e_S:.2e} (bound {4 * U:.2e})")
    assert e_S <= 4 * U
    ties = cot == 0.0
    assert ties.any() and (cot > 0).any() and (cot < 0).any()
    assert np.array_equal(c0 == 0.0, ties) and np.array_equal(np.sign(c0), np.sign(cot))  # exact 0 on ties, every sign exact
    e_c = np.abs(c0.astype(np.float64) - cot)[~ties] / np.abs(cot[~ties])
    print(f"    cotangents: max rel {e_c.max():.2e} (bound {2 * U:.2e}); ties {int(ties.sum())} of {3 * n}")
    assert e_c.max() <= 2 * U
    # summary4[3] += weight * S: from 0 within the bound on S; from 0.625 one more rounding of the sum
    assert list(s0[:3]) == [1.0, 2.0, 3.0] and abs(s0[3] - w32 * S) <= 4 * U * w32 * S
    assert list(s2[:3]) == [1.0, 2.0, 3.0] and abs(s2[3] - (0.625 + w32 * S)) <= 4 * U * w32 * S + 0.5 * U * abs(s2[3])
    assert l2.tobytes() == l0.tobytes() and c2.tobytes() == c0.tobytes()
    # without a summary the loss and the cotangents are the same
    loss = torch.zeros(1, device=dev)
    cot3 = torch.zeros(3 * n, device=dev)
    E.fd_smoothness(u3, eps, weight, loss, cot3, scratch)
    assert loss.cpu().numpy().tobytes() == l0.tobytes() and cot3.cpu().numpy().tobytes() == c0.tobytes()


def test_smoothness_on_misaligned_buffers_equals_the_aligned_call(dev):
    """Which thread sums which point does not depend on the alignment: the same bits from views that start 4 bytes in."""
    E = _E()
    from pinnrl_amd import _lib

    n, eps = 1027, 1e-4
    u3h = _values(n)
    scratch = torch.zeros(_lib.PINN_FD_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    out = []
    for offset in (0, 1):
        ub = torch.zeros(3 * n + 1, device=dev)
        cb = torch.zeros(3 * n + 1, device=dev)
        u3, cot3 = ub[offset : offset + 3 * n], cb[offset : offset + 3 * n]
        u3.copy_(torch.from_numpy(u3h))
        loss = torch.zeros(1, device=dev)
        E.fd_smoothness(u3, eps, 0.1, loss, cot3, scratch)
        out.append((loss.cpu().numpy().tobytes(), cot3.cpu().numpy().tobytes()))
    assert out[0] == out[1]


def test_bad_arguments_return_their_status_and_write_nothing(dev):
    E = _E()
    from pinnrl_amd import _lib

    lib = _lib.load()
    n = 37
    x, t = torch.rand(n, device=dev), torch.rand(n, device=dev)
    x3, t3 = torch.full((3 * n,), -7.0, device=dev), torch.full((3 * n,), -7.0, device=dev)
    st = E._stream(dev)
    px, pt, p3, q3 = x.data_ptr(), t.data_ptr(), x3.data_ptr(), t3.data_ptr()
    BAD = -1  # PINN_ERR_BAD_DESC
    with torch.cuda.device(dev):
        for args in ((px, pt, -1, 1e-4, LO, HI, p3, q3), (px, pt, n, 0.0, LO, HI, p3, q3), (px, pt, n, -1e-4, LO, HI, p3, q3),
                     (px, pt, n, float("nan"), LO, HI, p3, q3), (px, pt, n, 1e-4, HI, LO, p3, q3), (None, pt, n, 1e-4, LO, HI, p3, q3),
                     (px, None, n, 1e-4, LO, HI, p3, q3), (px, pt, n, 1e-4, LO, HI, None, q3), (px, pt, n, 1e-4, LO, HI, p3, None)):
            assert lib.pinn_fd_stencil_points(*args, st) == BAD, args
            assert "pinn_fd_stencil_points" in lib.pinn_last_error().decode()
        assert lib.pinn_fd_stencil_points(None, None, 0, 1e-4, LO, HI, None, None, st) == 0  # N == 0: a no-op
        assert lib.pinn_fd_stencil_points(px, pt, 0, 1e-4, LO, HI, p3, q3, st) == 0
    torch.cuda.synchronize()
    assert bool((x3 == -7.0).all()) and bool((t3 == -7.0).all())
    with torch.cuda.device(dev):
        assert lib.pinn_fd_stencil_points(px, pt, n, 1e-4, LO, LO, p3, q3, st) == 0  # lo == hi is a (degenerate) domain
    torch.cuda.synchronize()
    assert torch.equal(x3[:n], x) and bool((x3[n:] == LO).all())
    x3.fill_(-7.0)
    t3.fill_(-7.0)

    u3 = torch.rand(3 * n, device=dev)
    loss, cot3 = torch.full((1,), -7.0, device=dev), torch.full((3 * n,), -7.0, device=dev)
    summary = torch.full((4,), -7.0, device=dev)
    scratch = torch.full((_lib.PINN_FD_SCRATCH_DOUBLES + 1,), -7.0, dtype=torch.float64, device=dev)
    pu, pl, pc, ps, pk = u3.data_ptr(), loss.data_ptr(), cot3.data_ptr(), summary.data_ptr(), scratch.data_ptr()
    with torch.cuda.device(dev):
        for args in ((pu, 0, 1e-4, 0.1, pl, pc, ps, pk), (pu, -n, 1e-4, 0.1, pl, pc, ps, pk), (pu, n, 0.0, 0.1, pl, pc, ps, pk),
                     (pu, n, -1.0, 0.1, pl, pc, ps, pk), (None, n, 1e-4, 0.1, pl, pc, ps, pk), (pu, n, 1e-4, 0.1, None, pc, ps, pk),
                     (pu, n, 1e-4, 0.1, pl, None, ps, pk), (pu, n, 1e-4, 0.1, pl, pc, ps, None)):
            assert lib.pinn_fd_smoothness(*args, st) == BAD, args
            assert "pinn_fd_smoothness" in lib.pinn_last_error().decode()
        assert lib.pinn_fd_smoothness(pu, n, 1e-4, 0.1, pl, pc, ps, pk + 4, st) == -3  # PINN_ERR_MISALIGNED
    torch.cuda.synchronize()
    for buf in (x3, t3, loss, cot3, summary, scratch):
        assert bool((buf == -7.0).all())
