"""CPU tests (no GPU) of HeatEquation's finite-difference smoothness term on the autograd-free step.

(a) the fp64 model of tests/smoothness_model.py against torch fp64 autograd of the restated reference formula
    (pinnrl/pdes/heat_equation.py:625-650), exact ties on the domain ends included; its fp32 stencil points against torch;
(b) the conditioning of the term at the reference's eps = 1e-4 and at eps = 2^-6, fp32 against fp64, on the project's
    network (printed: the figures behind the tolerances of tests/test_smoothness_step_gpu.py);
(c) routing: `_manual_step_unsupported()` on a CPU-built trainer, and `_manual_smoothness()`;
(d) the new symbols are declared, listed and exported;
(e) the host logic of the launch list with the smoothness chain under an oracle-backed CPU stand-in for the engine."""

import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_case, rel_l2

import oracle as O
import smoothness_model as SM

import pinnrl_amd  # noqa: F401
from pinnrl_amd import _lib
from pinnrl_amd import pdes as P
from pinnrl_amd.config import AdaptiveWeightsConfig, Config, TrainingConfig
from pinnrl_amd.training import PDETrainer

LO, HI, T_MAX = 0.0, 2.0, 10.0
REF_WEIGHTS = {"residual": 15.0, "boundary": 20.0, "initial": 10.0, "smoothness": 0.1}  # the reference's default configuration


def _jittered_batch(seed=0, side=31, on_each_end=14):
    """side^2 jittered-grid points on [LO, HI] x [0, T_MAX], fp32, `on_each_end` of them exactly on either domain end."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(side, dtype=torch.float64)
    gx, gt = torch.meshgrid(i, i, indexing="ij")
    x = (LO + (gx + torch.rand(side, side, generator=g, dtype=torch.float64)) * (HI - LO) / side).reshape(-1, 1).float()
    t = ((gt + torch.rand(side, side, generator=g, dtype=torch.float64)) * T_MAX / side).reshape(-1, 1).float()
    perm = torch.randperm(side * side, generator=g)
    x[perm[:on_each_end]] = LO
    x[perm[on_each_end : 2 * on_each_end]] = HI
    return x.contiguous(), t.contiguous()


def _restated(model_fn, x, t, eps, dtype):
    """The reference formula in plain torch at `dtype`: the points are formed in fp32 (they are fp32 tensors in the
    reference), the network and the term run at `dtype`."""
    xp = torch.clamp(x + eps, LO, HI)
    xm = torch.clamp(x - eps, LO, HI)
    assert xp.dtype == torch.float32
    uc, up, um = (model_fn(torch.cat([p, t], 1).to(dtype)) for p in (x, xp, xm))
    return torch.mean(torch.abs((up - uc) / eps)) + torch.mean(torch.abs((uc - um) / eps)), (uc, up, um)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-4, 2.0**-6])
def test_stencil_points_of_the_model_are_torchs(eps):
    x, t = _jittered_batch()
    x3, t3 = SM.stencil_points(x.numpy(), t.numpy(), eps, LO, HI)
    want = torch.cat([x, torch.clamp(x + eps, LO, HI), torch.clamp(x - eps, LO, HI)]).reshape(-1)
    assert torch.equal(torch.from_numpy(x3), want) and torch.equal(torch.from_numpy(t3), torch.cat([t, t, t]).reshape(-1))
    n = x.shape[0]
    assert int((x3[n : 2 * n] == x3[:n]).sum()) == 14 and int((x3[2 * n :] == x3[:n]).sum()) == 14  # the clamp ties the end points


@pytest.mark.parametrize("case", ["burgers_fourier_3x32", "burgers_feedforward_3x32"])
@pytest.mark.parametrize("eps", [1e-4, 2.0**-6])
def test_model_equals_fp64_autograd_of_the_restated_formula(case, eps):
    spec, _, sd, _, _ = load_case(case)
    x, t = _jittered_batch()
    p64 = {k: v.double().requires_grad_(not k.endswith("fourier.B")) for k, v in sd.items()}
    names = [k for k in p64 if p64[k].requires_grad]
    S, (uc, up, um) = _restated(lambda z: O.network_forward(spec, p64, z), x, t, eps, torch.float64)
    weight = 0.1
    grads = torch.autograd.grad(weight * S, [p64[k] for k in names] + [uc, up, um], retain_graph=False)
    got_S, got_g, u3 = SM.term_and_weight_gradient(spec, sd, x.numpy(), t.numpy(), eps, LO, HI, weight)
    assert abs(got_S - float(S.detach())) <= 1e-12 * abs(float(S.detach()))
    e = rel_l2(torch.cat([got_g[k].flatten() for k in names]), torch.cat([g.flatten() for g in grads[: len(names)]]))
    assert e <= 1e-10, e
    # S and the cotangents from given values: autograd's d(weight S)/d(uc, up, um), ties included (sgn(0) = 0)
    S2, cot = SM.smoothness_terms(u3, eps, weight)
    want_cot = torch.cat([g.flatten() for g in grads[len(names) :]]).numpy()
    assert S2 == got_S and np.array_equal(cot == 0.0, want_cot == 0.0)
    assert np.abs(cot - want_cot).max() <= 1e-12 * np.abs(want_cot).max()
    n = x.shape[0]
    ends = (x.reshape(-1) == LO) | (x.reshape(-1) == HI)
    assert int(ends.sum()) == 28 and (cot[n : 2 * n][(x.reshape(-1) == HI).numpy()] == 0).all()
    assert (cot[2 * n :][(x.reshape(-1) == LO).numpy()] == 0).all()


def test_model_handles_planted_values():
    u3 = np.array([1.0, 2.0, 3.0, 4.0, 1.5, 2.0, 2.0, 4.0, 1.0, 2.5, 3.0, 3.0], dtype=np.float32)  # uc | up | um, N = 4
    S, cot = SM.smoothness_terms(u3, 0.5, 2.0)
    assert S == (0.5 + 0.0 + 1.0 + 0.0) / 0.5 / 4 + (0.0 + 0.5 + 0.0 + 1.0) / 0.5 / 4
    c = 2.0 / (0.5 * 4)
    assert np.array_equal(cot, c * np.array([-1, -1, 1, 1, 1, 0, -1, 0, 0, 1, 0, -1], dtype=np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# (b) conditioning (printed; what is asserted is only what is well-defined at either eps)
# ---------------------------------------------------------------------------------------------------------------------
def test_conditioning_of_the_reference_term_in_fp32():
    spec, _, sd, _, _ = load_case("burgers_fourier_3x32")
    x, t = _jittered_batch()
    names = [k for k in sd if not k.endswith("fourier.B")]
    for eps in (1e-4, 2.0**-6):
        S64, g64, u64 = SM.term_and_weight_gradient(spec, sd, x.numpy(), t.numpy(), eps, LO, HI)
        w64 = torch.cat([g64[k].flatten() for k in names])
        out = {}
        for tag, perm in (("fp32", torch.arange(x.shape[0])), ("fp32 permuted", torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(1)))):
            p32 = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
            S32, (uc, up, um) = _restated(lambda z: O.network_forward(spec, p32, z), x[perm], t[perm], eps, torch.float32)
            g32 = torch.autograd.grad(S32, [p32[k] for k in names])
            inv = torch.argsort(perm)
            out[tag] = (float(S32.detach()), torch.cat([g.flatten() for g in g32]), torch.cat([uc[inv], up[inv], um[inv]]).reshape(-1).detach())
        S32, w32, u32 = out["fp32"]
        n = x.shape[0]
        s32 = torch.cat([torch.sign(u32[n : 2 * n] - u32[:n]), torch.sign(u32[:n] - u32[2 * n :])]).numpy()
        s64 = np.concatenate([np.sign(u64[n : 2 * n] - u64[:n]), np.sign(u64[:n] - u64[2 * n :])])
        print(f"eps {eps:.3e}: S fp32 vs fp64 {abs(S32 - S64) / S64:.2e}; weight gradient fp32 vs fp64 {rel_l2(w32, w64):.2e}; "
              f"fp32 vs itself, batch permuted {rel_l2(out['fp32 permuted'][1], w32):.2e}; sign flips {int((s32 != s64).sum())} of {2 * n}; "
              f"exact ties {int((s64 == 0).sum())}")
        assert int((s64 == 0).sum()) == 28 and int((s32 == 0).sum()) >= 28  # the clamp's ties are exact in any precision


# ---------------------------------------------------------------------------------------------------------------------
# (c) routing
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(weights=REF_WEIGHTS, **training):
    cfg = Config.__new__(Config)
    cfg.device = torch.device("cpu")
    cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, weight_decay=5e-4, loss_weights=dict(weights), **training)
    return cfg


def _obs():
    g = torch.Generator().manual_seed(0)
    return {"x": torch.rand(20, 1, generator=g) * 2, "t": torch.rand(20, 1, generator=g) * 10, "u": torch.rand(20, 1, generator=g)}


def _heat(cfg, cls=P.HeatEquation, dimension=1, trainable=(), obs=None):
    return cls(P.PDEConfig(
        name="heat", domain=[(LO, HI)] * dimension, time_domain=(0.0, T_MAX), parameters={"alpha": 0.01},
        boundary_conditions={"periodic": {}}, initial_condition={"type": "sine", "amplitude": 1.0, "frequency": 2.0},
        exact_solution={}, dimension=dimension, device=torch.device("cpu"), training=cfg.training,
        trainable_parameters=list(trainable), parameter_initial_guesses={"alpha": 0.02} if trainable else {}, observation_data=obs))


def _trainer(cfg, **pde_kw):
    dim = pde_kw.get("dimension", 1)
    return PDETrainer(torch.nn.Linear(dim + 1, 1), _heat(cfg, **pde_kw), {}, cfg, device=torch.device("cpu"))


def test_heat_with_the_reference_loss_weights_takes_the_launch_list():
    assert _trainer(_cfg())._manual_step_unsupported() is None  # the parent: "smoothness term"
    assert _trainer(_cfg(optimizer="lbfgs"))._manual_step_unsupported() is None
    assert _trainer(_cfg(optimizer="adam_lbfgs"))._manual_step_unsupported() is None
    assert _trainer(_cfg(mode="inverse"), trainable=["alpha"], obs=_obs())._manual_step_unsupported() is None
    assert _trainer(_cfg(mode="data_augmented"), obs=_obs())._manual_step_unsupported() is None


def test_what_stays_on_the_autograd_step_names_the_smoothness_term():
    cfg = _cfg()
    cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy="rbw")
    why = _trainer(cfg)._manual_step_unsupported()
    assert isinstance(why, str) and "smoothness" in why and "adaptive" in why

    class OwnLoss(P.HeatEquation):  # an own compute_loss with a launch-list chain, but no launch-list form of its smoothness term
        _manual_smoothness = P.PDEBase._manual_smoothness

    assert _trainer(_cfg(), cls=OwnLoss)._manual_step_unsupported() == "smoothness term"
    weights = dict(REF_WEIGHTS, smoothness=0.0)
    assert _trainer(_cfg(weights), cls=OwnLoss)._manual_step_unsupported() is None

    tr = _trainer(_cfg())
    tr.process_group = object()
    assert tr._manual_step_unsupported() == "smoothness term under a process group"
    tr.process_group = None
    assert tr._manual_step_unsupported() is None

    assert _trainer(_cfg(), dimension=2)._manual_step_unsupported() == "smoothness term"


def test_manual_smoothness_values():
    sm = _heat(_cfg())._manual_smoothness()
    assert sm == {"eps": 1e-4, "weight": 0.1, "lo": LO, "hi": HI}
    assert P.HeatEquation._SMOOTHNESS_EPS == 1e-4
    assert _heat(_cfg(), dimension=2)._manual_smoothness() is None
    assert _heat(_cfg(dict(REF_WEIGHTS, smoothness=0.0)))._manual_smoothness() is None
    no_key = {k: v for k, v in REF_WEIGHTS.items() if k != "smoothness"}
    assert _heat(_cfg(no_key))._manual_smoothness() is None
    assert P.PDEBase._manual_smoothness(_heat(_cfg())) is None

    class Wider(P.HeatEquation):
        _SMOOTHNESS_EPS = 2.0**-6

    assert _heat(_cfg(), cls=Wider)._manual_smoothness()["eps"] == 2.0**-6


def test_the_eager_term_reads_the_class_attribute():
    """`_compute_smoothness_loss` at the attribute's eps equals the restated formula (same ops, same order: bit for bit)."""
    spec, _, sd, _, _ = load_case("burgers_fourier_3x32")
    x, t = _jittered_batch()
    model = lambda z: O.network_forward(spec, sd, z)  # noqa: E731
    for eps, cls in ((1e-4, P.HeatEquation), (2.0**-6, type("Wider", (P.HeatEquation,), {"_SMOOTHNESS_EPS": 2.0**-6}))):
        got = _heat(_cfg(), cls=cls)._compute_smoothness_loss(model, x, t)
        want, _ = _restated(model, x, t, eps, torch.float32)
        assert float(got) == float(want)


# ---------------------------------------------------------------------------------------------------------------------
# (d) exports
# ---------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "pinn_jet.h")) as f:
        header = f.read()
    assert "int pinn_fd_stencil_points(" in header and "int pinn_fd_smoothness(" in header
    assert f"#define PINN_FD_SCRATCH_DOUBLES {_lib.PINN_FD_SCRATCH_DOUBLES}" in header
    assert "pinn_fd_stencil_points" in _lib.EXPORTS and "pinn_fd_smoothness" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.pinn_fd_stencil_points.argtypes is not None and lib.pinn_fd_smoothness.argtypes is not None
    assert _lib.PINN_ABI_VERSION == 2 and lib.pinn_abi_version() == 2  # an additive change


# ---------------------------------------------------------------------------------------------------------------------
# (e) host logic of the launch list with the smoothness chain, engine replaced by an oracle-backed CPU stand-in (the
#     pattern of tests/test_distributed_cpu.py) against the fp64 model of the whole step
# ---------------------------------------------------------------------------------------------------------------------
import test_distributed_cpu as tdc  # noqa: E402
import train_step_model as TS  # noqa: E402
from pinnrl_amd.training import trainer as T  # noqa: E402


class _HeatEngine(tdc._FakeEngine):
    """`tdc._FakeEngine` for HeatEquation's chain — (u, u_t, u_x) jets by autograd, paired terms — plus the two new calls
    in the arithmetic of the entry points (fp32 stencil points, S and cotangents from the fp32 values)."""

    pde_spec = O.PdeSpec(name="heat", parameters={"alpha": 0.01}, domain=[(LO, HI)], time_domain=(0.0, T_MAX))
    calls = []

    @classmethod
    def residual_loss_grad(cls, prog, pd, x, t, scale, flat, want_residual=False, loss_sum=None):
        ps = [p for p, tr in zip(prog.tensors, prog.trainable) if tr]
        with torch.enable_grad():
            r = O.compute_residual(cls.pde_spec, cls._fn(prog), x, t)
            L = (r**2).sum()
            gs = torch.autograd.grad(L * scale, ps, allow_unused=True)  # u_t - alpha u_x does not see the output bias
        cls._accumulate(prog, flat, [g if g is not None else torch.zeros_like(p) for g, p in zip(gs, ps)])
        loss_sum += L.detach()
        return None, loss_sum

    @classmethod
    def _jets(cls, prog, x, t, nt, nx, create_graph):
        x, t = x.detach().clone().requires_grad_(True), t.detach().clone().requires_grad_(True)
        u = cls._fn(prog)(torch.cat([x, t], 1))
        out = [u]
        if nt:
            out.append(torch.autograd.grad(u.sum(), t, create_graph=create_graph, retain_graph=True)[0])
        if nx:
            out.append(torch.autograd.grad(u.sum(), x, create_graph=create_graph, retain_graph=True)[0])
        return torch.stack([s.reshape(-1) for s in out])

    @classmethod
    def jets_forward(cls, prog, x, t, nt, nx):
        cls.calls.append(("jets_forward", x.shape[0], nt, nx))
        with torch.enable_grad():
            return cls._jets(prog, x, t, nt, nx, False).detach()

    @classmethod
    def jets_backward(cls, prog, x, t, nt, nx, cot, flat):
        cls.calls.append(("jets_backward", x.shape[0], nt, nx))
        ps = [p for p, tr in zip(prog.tensors, prog.trainable) if tr]
        with torch.enable_grad():
            gs = torch.autograd.grad((cls._jets(prog, x, t, nt, nx, True) * cot).sum(), ps)
        cls._accumulate(prog, flat, gs)

    @classmethod
    def jet_losses(cls, jets, terms, loss, huber_delta, term_losses, cot, residual_sum=None, residual_scale=0.0, residual_weight=0.0,
                   n_boundary_terms=0, summary4=None):
        cls.calls.append(("jet_losses",))
        np_terms = [(lo, hi, st, pr, None if tg is None else tg.numpy(), w) for lo, hi, st, pr, tg, w in terms]
        L, c, summary = TS.jet_loss_terms(jets.numpy(), np_terms, loss, huber_delta, residual_sum=float(residual_sum[0]),
                                          residual_scale=residual_scale, residual_weight=residual_weight, n_boundary_terms=n_boundary_terms)
        term_losses.copy_(torch.from_numpy(L).float())
        cot.copy_(torch.from_numpy(c).float())
        if summary4 is not None:
            summary4.copy_(torch.from_numpy(summary).float())

    @classmethod
    def fd_stencil_points(cls, x, t, eps, lo, hi, x3, t3):
        cls.calls.append(("fd_stencil_points", x.numel()))
        assert x.dim() == 1 and x.is_contiguous() and x3.numel() == 3 * x.numel() == t3.numel()
        a, b = SM.stencil_points(x.numpy(), t.numpy(), eps, lo, hi)
        x3.copy_(torch.from_numpy(a).view_as(x3))
        t3.copy_(torch.from_numpy(b).view_as(t3))

    @classmethod
    def fd_smoothness(cls, u3, eps, weight, loss_out, cot3, scratch, summary4=None):
        cls.calls.append(("fd_smoothness", u3.numel()))
        S, cot = SM.smoothness_terms(u3.numpy(), eps, weight)
        loss_out[0] = S
        cot3.copy_(torch.from_numpy(cot).float().view_as(cot3))
        if summary4 is not None:
            summary4[3] += weight * S


class _OracleHeat(P.HeatEquation):
    _SMOOTHNESS_EPS = 2.0**-6


@pytest.mark.parametrize("smoothness", [0.1, 0.0])
def test_launch_list_host_logic_against_the_fp64_step_model(smoothness, monkeypatch):
    spec, _, sd, _, _ = load_case("burgers_fourier_3x32")
    _HeatEngine.spec, _HeatEngine.calls = spec, []
    monkeypatch.setattr(T, "_E", _HeatEngine)
    cfg = _cfg(dict(REF_WEIGHTS, smoothness=smoothness))
    model = tdc._ManualOracleModel(spec, sd)
    pde = _heat(cfg, cls=_OracleHeat)
    tr = PDETrainer(model, pde, {}, cfg, device=torch.device("cpu"))
    assert tr._manual_step_unsupported() is None
    tr._build_flat_state()
    x, t = _jittered_batch(side=15, on_each_end=6)
    n = x.shape[0]
    losses = tr.train_step(x, t)
    F = tr._flat
    ch = pde._manual_chain(n)
    terms = [(lo, hi, st, pr, None if tg is None else tg.numpy(), w) for lo, hi, st, pr, tg, w in ch["terms"]]
    sm = {"eps": 2.0**-6, "weight": smoothness, "lo": LO, "hi": HI} if smoothness > 0 else None
    want, grads, _ = SM.heat_step(spec, sd, x.numpy(), t.numpy(), 0.01, 15.0, ch["x"].numpy(), ch["t"].numpy(), terms, ch["n_bc"], sm)
    names = [k for k in sd if not k.endswith("fourier.B")]
    prog = model.program()
    offs, _ = prog.grad_layout()
    got = torch.cat([F["grad"][o : o + p.numel()] for p, o in zip(prog.tensors, offs) if o >= 0])  # the layout pads to 16 bytes
    e = rel_l2(got, torch.cat([grads[k].flatten() for k in names]))
    assert e <= 1e-5, e
    for k in ("residual", "boundary", "initial", "total") + (("smoothness",) if sm else ()):
        assert abs(float(losses[k]) - want[k]) <= 1e-5 * abs(want[k]), (k, float(losses[k]), want[k])
    kinds = [c[0] for c in _HeatEngine.calls]
    if sm:
        # after the boundary / initial chain: stencil points, values on 3 n points, S + cotangents, the reverse sweep
        assert kinds == ["jets_forward", "jet_losses", "jets_backward", "fd_stencil_points", "jets_forward", "fd_smoothness", "jets_backward"]
        assert _HeatEngine.calls[4] == ("jets_forward", 3 * n, 0, 0) and _HeatEngine.calls[6] == ("jets_backward", 3 * n, 0, 0)
        assert set(F["chains"][(n, 1)]["smooth"]) >= {"x3", "t3", "cot3", "scratch", "eps", "weight", "lo", "hi"}
        assert abs(float(losses["total"]) - (want["total"] - smoothness * want["smoothness"]) - smoothness * float(losses["smoothness"])) <= 1e-5
    else:  # weight 0: no new buffers, no new launches, no new key
        assert kinds == ["jets_forward", "jet_losses", "jets_backward"]
        assert "smooth_loss" not in F and "smooth" not in F["chains"][(n, 1)] and "smoothness" not in losses


def test_argument_checks_run_on_the_host_before_any_launch():
    """Every refusal returns its PinnStatus from the host-side checks: no device is needed (none is present here)."""
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned stand-in for a device pointer: a refused call reads nothing
    for args in ((p, p, -1, 1e-4, LO, HI, p, p), (p, p, 8, 0.0, LO, HI, p, p), (p, p, 8, -1e-4, LO, HI, p, p),
                 (p, p, 8, float("nan"), LO, HI, p, p), (p, p, 8, 1e-4, HI, LO, p, p), (None, p, 8, 1e-4, LO, HI, p, p),
                 (p, None, 8, 1e-4, LO, HI, p, p), (p, p, 8, 1e-4, LO, HI, None, p), (p, p, 8, 1e-4, LO, HI, p, None)):
        assert lib.pinn_fd_stencil_points(*args, None) == -1, args  # PINN_ERR_BAD_DESC
        assert "pinn_fd_stencil_points" in lib.pinn_last_error().decode()
    assert lib.pinn_fd_stencil_points(None, None, 0, 1e-4, LO, HI, None, None, None) == 0  # N == 0: a no-op
    for args in ((p, 0, 1e-4, 0.1, p, p, p, p), (p, -8, 1e-4, 0.1, p, p, p, p), (p, 8, 0.0, 0.1, p, p, p, p), (p, 8, -1.0, 0.1, p, p, p, p),
                 (None, 8, 1e-4, 0.1, p, p, p, p), (p, 8, 1e-4, 0.1, None, p, p, p), (p, 8, 1e-4, 0.1, p, None, p, p),
                 (p, 8, 1e-4, 0.1, p, p, p, None)):
        assert lib.pinn_fd_smoothness(*args, None) == -1, args
        assert "pinn_fd_smoothness" in lib.pinn_last_error().decode()
    assert lib.pinn_fd_smoothness(p, 8, 1e-4, 0.1, p, p, None, p + 4, None) == -3  # PINN_ERR_MISALIGNED: scratch
