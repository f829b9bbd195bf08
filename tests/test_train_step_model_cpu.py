"""The fp64 models of tests/train_step_model.py pinned on the CPU: FlatAdam against torch.optim.Adam + clip_grad_norm_ on an
fp64 parameter, the loss-term model against formulas written out by hand, and the fp32 yardstick against FlatAdam."""

import numpy as np
import pytest
import torch

import train_step_model as TM
from adaptive_model import FlatAdam


@pytest.mark.parametrize("wd,max_norm", [(0.0, 0.0), (1e-2, 1.0), (1e-2, 0.5)])
def test_flat_adam_is_torch_adam_with_clipping(wd, max_norm):
    """20 steps, theta_0 ~ N(0, 1), 53 elements with gradient norms around 7 (both clip settings are active).  Measured
    agreement: <= 3e-16 relative."""
    rng = np.random.default_rng(11)
    theta0 = rng.standard_normal(53)
    p = torch.nn.Parameter(torch.from_numpy(theta0.copy()))
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    flat = FlatAdam(theta0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, max_norm=max_norm)
    for step in range(20):
        g = rng.standard_normal(53)
        p.grad = torch.from_numpy(g.copy())
        want_norm = float(p.grad.norm())
        if max_norm > 0:
            assert want_norm > 2.0 * max_norm
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        _, norm = flat.step(g[None, :], [1.0])
        assert abs(norm - want_norm) <= 1e-12 * want_norm
        st = opt.state[p]
        for name, got, want in (("theta", flat.theta, p.detach()), ("m", flat.m, st["exp_avg"]), ("v", flat.v, st["exp_avg_sq"])):
            e = TM.rel_l2_np(got, want.numpy())
            assert e <= 1e-12, (step, name, e)
        assert flat.t == int(st["step"])


def _by_hand(r, loss, d):
    """(mean l(r), l'(r) / len(r)) written out."""
    if loss == "mse":
        return np.mean(r * r), 2.0 * r / r.size
    if loss == "mae":
        return np.mean(np.abs(r)), np.sign(r) / r.size
    quad = np.abs(r) <= d
    return np.mean(np.where(quad, 0.5 * r * r, d * (np.abs(r) - 0.5 * d))), np.where(quad, r, d * np.sign(r)) / r.size


@pytest.mark.parametrize("loss", ["mse", "mae", "huber"])
def test_loss_model_against_hand_written_formulas(loss):
    """One paired term on stream 1 and one target term on stream 0, with a zero difference and |difference| == delta planted
    in each; an uncovered tail."""
    rng = np.random.default_rng(5)
    d, n, h = 0.25, 20, 6
    J = rng.standard_normal((2, n))
    target = rng.standard_normal(7)
    J[0, 3], J[0, 4], J[0, 5] = target[0], target[1] + d, target[2] - d  # the target term covers [3, 10)
    J[1, 0], J[1, 1] = J[1, h], J[1, h + 1] + d
    w_pair, w_tg, rsum, rscale, rw = 0.75, 1.5, 3.0, 0.125, 2.0
    terms = [(0, h, 1, h, None, w_pair), (3, 10, 0, 0, target, w_tg)]
    L, cot, summary = TM.jet_loss_terms(J, terms, loss, d, residual_sum=rsum, residual_scale=rscale, residual_weight=rw,
                                        n_boundary_terms=1)
    lp, gp = _by_hand(J[1, :h] - J[1, h : 2 * h], loss, d)
    lt, gt = _by_hand(J[0, 3:10] - target, loss, d)
    want = np.zeros_like(J)
    want[1, :h], want[1, h : 2 * h] = w_pair * gp, -w_pair * gp
    want[0, 3:10] = w_tg * gt
    assert np.allclose(L, [lp, lt], rtol=1e-14, atol=0.0)
    assert np.allclose(cot, want, rtol=1e-14, atol=1e-300)
    assert np.all(cot[0, 10:] == 0.0) and np.all(cot[1, 2 * h :] == 0.0) and np.all(cot[0, :3] == 0.0)
    assert cot[0, 3] == 0.0 and cot[1, 0] == 0.0 and cot[1, h] == 0.0  # zero difference: no cotangent under every loss
    assert np.allclose(summary, [rsum * rscale, lp, lt, rw * rsum * rscale + w_pair * lp + w_tg * lt], rtol=1e-14, atol=0.0)
    # the K = 1 form, no residual
    L1, cot1, s1 = TM.point_loss_terms(J[0], [(3, 10, target, w_tg)], loss, d, n_boundary_terms=1)
    assert np.allclose(L1, [lt], rtol=1e-14) and np.allclose(cot1, want[0], rtol=1e-14, atol=1e-300)
    assert np.allclose(s1, [0.0, lt, 0.0, w_tg * lt], rtol=1e-14)


def test_loss_model_empty_term_and_no_terms():
    J = np.random.default_rng(1).standard_normal((2, 9))
    L, cot, s = TM.jet_loss_terms(J, [(4, 4, 1, 0, np.zeros(1), 2.0), (0, 3, 0, 0, np.zeros(3), 1.0)], "mse", 1.0, n_boundary_terms=1)
    assert L[0] == 0.0 and np.all(cot[1] == 0.0) and np.isfinite(cot).all() and s[1] == 0.0 and s[2] == L[1]
    L, cot, s = TM.jet_loss_terms(J, [], "mae", 1.0, residual_sum=8.0, residual_scale=0.5, residual_weight=3.0)
    assert L.size == 0 and np.all(cot == 0.0) and s.tolist() == [4.0, 0.0, 0.0, 12.0]


def test_fp32_yardstick_follows_flat_adam():
    """The specified formulas in numpy fp32 against FlatAdam, theta_0 = 0, n = 16 387, twelve steps from step 0 and twelve from
    step 9 999: theta stays at the fp32 floor (measured 0.8-1.2e-7).  With `1 - b**t` in fp32 for the bias corrections, steps
    2-12 of the first sequence sit at 0.65-1.5e-6 instead."""
    n = 16387
    for t0 in (0, 9999):
        rng = np.random.default_rng(n + t0)
        m0 = 0.1 * rng.standard_normal(n).astype(np.float32) if t0 else None
        v0 = rng.uniform(0.5, 1.5, n).astype(np.float32) if t0 else None
        hp = dict(weight_decay=1e-2, max_norm=1.0, m=m0, v=v0, t=t0)
        a64, a32 = TM.make_adam(n, **hp), TM.AdamFp32(n, **hp)
        for step in range(12):
            g = rng.standard_normal(n).astype(np.float32)
            norm = TM.adam_step(a64, g)
            norm32 = a32.step(g)
            assert abs(norm32 - norm) <= 1e-6 * norm
            for name, got, want in (("theta", a32.theta, a64.theta), ("m", a32.m, a64.m), ("v", a32.v, a64.v)):
                e = TM.rel_l2_np(got, want)
                assert e <= 3e-7, (t0, step, name, e)
        assert float(a32.t) == a64.t == t0 + 12
