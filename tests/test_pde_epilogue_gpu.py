"""GPU: every cell of the PDE epilogue (`csrc/jet_device.h`: pde_residual, pde_coef_grads, loss_term) on every kernel family
that instantiates it, against the fp64 reference of tests/epilogue_cells.py.

Lanes: `lm` (the layer-major head, and the by-value coefficient path on it), `wide64` (the 32-point kernel at image height
64: every stream set), `wide128` (the 32-point kernel at height 128), `u16` (the 16-point units; Burgers on the merged
units) and `u16_plain` (Burgers on the four-stream units).  The kernel every call takes is asserted through the queries.
Per (cell, lane, loss kind): `residual_forward`, `residual_loss_grad`, `residual_loss_grad_inverse` (coefficients from a
device array, `pde.coef` garbage); per (cell, lane): `residual_backward` with a fixed cotangent and one inverse call under
PINN_FLAG_DETERMINISTIC.  50 points: a full tile / three full units and a ragged tail.  The cached workspaces are filled
with NaN before every reverse launch.

Bars (the ones the project holds these quantities to): residual, loss and concatenated weight gradient 1e-5
(tests/test_hip_parity.py; 2e-5 for the gradient under mae / huber), per-tensor gradients through
`hip_helpers.check_tensors`, coefficient gradients |got - want| <= 2e-5 |want| + 1e-9 (tests/test_inverse_fused_gpu.py);
whatever vanishes identically in the reference must be exactly 0.  Nothing is excluded from a comparison.

Found by this file: on the (1,0) 16-point tanh unit (every >= 2-D cell but wave and pendulum on the `u16` lane) the fused call's
residuals differed from the forward-only call's by up to 512 ulp of a small u_t, against the promise of
csrc/jet_kernel_u16.h: the compiler contracted 1 - y * y of the tanh jets to an fma in one instantiation and not in the
other (csrc/jet_device.h::act_derivs now spells the fma out at first order; profiles/parity_pde_epilogue.md)."""

import ctypes
import json
import os
import time

import pytest
import torch

import epilogue_cells as C
from conftest import _PARITY_LOG, rel_err, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
COEF_TOL = 2e-5
GARBAGE = (-7.5e3, 1.0e9, float("nan"), -3.0)  # tests/test_inverse_fused_gpu.py: the inverse call must not read pde->coef

_RAN = []      # (cell id, lane, unit, inverse kernel) of every case that ran
_WORST = {}    # lane -> {quantity: (value, where)}
_WIDENED = []  # tensors that took check_tensors' fp32-floor bar
_T0 = time.time()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _stop_at_the_first_gpu_error():
    """A HIP error ends the run of this file: nothing more is launched on a device that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, stopping: {e}", returncode=3)


def _poison(prog, pd, dev, nt, nx):
    """Size the cached workspace for the forward-mode and the inverse call, then fill every cached workspace with NaN."""
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    lib = _lib.load()
    nbytes = max(lib.pinn_workspace_bytes(ctypes.byref(prog.desc), C.N, nt, nx, 1),
                 lib.pinn_inverse_workspace_bytes(ctypes.byref(prog.desc), ctypes.byref(pd), C.N))
    if nbytes:
        E._workspace(dev, nbytes)
    for ws in E._workspaces.values():
        ws.view(torch.float32).fill_(float("nan"))


def _note(lane, what, value, where):
    w = _WORST.setdefault(lane, {})
    if what not in w or value > w[what][0]:
        w[what] = (value, where)


def _by_name(prog, names, flat):
    from pinnrl_amd import engine as E

    return {n: g for n, g in zip(names, E.split_flat_grad(prog, flat)) if g is not None}


def _check_theta(tag, lane, prog, names, flat, want, tol, floor):
    """Concatenated and per-tensor weight gradient against {name: fp64 gradient}."""
    from hip_helpers import check_tensors

    assert torch.isfinite(flat).all(), f"{tag}: non-finite weight gradient"
    got = _by_name(prog, names, flat)
    assert set(got) == set(want), tag
    e = rel_l2(torch.cat([got[k].flatten().cpu() for k in want]), torch.cat([want[k].flatten() for k in want]),
               label=f"{tag} weight gradient", tol=tol)
    _note(lane, "gradient", e, tag)
    assert e <= tol, f"{tag}: weight gradient rel l2 {e:.2e} > {tol:.0e}"
    _WIDENED.extend(check_tensors(got, want, tag, floor=floor))
    return e


def _check_residual(tag, lane, r, s, ref, loss):
    assert torch.isfinite(r).all() and torch.isfinite(s).all(), f"{tag}: non-finite residual or loss sum"
    er = rel_l2(r.cpu(), ref["r"], label=f"{tag} residual", tol=TOL)
    el = rel_err(float(s) / C.N, ref[loss]["L"], label=f"{tag} loss", tol=TOL)
    _note(lane, "residual", er, tag)
    _note(lane, "loss", el, tag)
    assert er <= TOL, f"{tag}: residual rel l2 {er:.2e}"
    assert el <= TOL, f"{tag}: loss rel err {el:.2e}"
    return er, el


def _check_coef(tag, lane, cg, want):
    """cg: the 4 (inverse call) or 2 (by-value call) floats the launch accumulated into zeros."""
    assert torch.isfinite(cg).all(), f"{tag}: non-finite coefficient gradient"
    for k, w in enumerate(want):
        g = float(cg[k])
        if w == 0.0:  # the reference's derivative vanishes identically
            assert g == 0.0, f"{tag}: d loss / d c{k} = {g!r} must be exactly 0"
            continue
        _note(lane, "coefficient", abs(g - w) / abs(w), tag)
        assert abs(g - w) <= COEF_TOL * abs(w) + 1e-9, f"{tag}: d loss / d c{k}: {g!r} vs {w!r}"
    assert all(float(v) == 0.0 for v in cg[2:]), f"{tag}: slots 2, 3 of coef_grads were written"


@pytest.mark.parametrize("kind,dim,lane", C.CASES, ids=[f"{C.cell_id(k, d)}-{lane}" for k, d, lane in C.CASES])
def test_cell(kind, dim, lane, dev):
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    net = C.LANE_NET[lane]
    ref = C.reference(kind, dim, net)
    cid = C.cell_id(kind, dim)
    prog, names = program_from_spec(ref["spec"], ref["sd"], dev)
    C.apply_lane(prog, lane)
    nt, nx = C.streams(kind, dim)
    q = C.route(prog, kind, dim)
    assert q == C.route(C.descriptor(lane, dim), kind, dim), "the descriptor-only program of the lane is not this program's descriptor"
    fam, inv = C.family(q["unit"]), C.family(q["inverse"])
    print(f"{cid} {lane}: forward {q['forward']}, unit {q['unit']}, inverse {q['inverse']}")
    x, t = ref["x"].to(dev), ref["t"].to(dev)
    cv = torch.tensor(list(C.coef_values(kind)) + [0.0, 0.0], dtype=torch.float32, device=dev)
    scale = 1.0 / C.N
    floor = lambda which: (lambda: C.fp32_floor(kind, dim, net, which))  # noqa: E731

    def inverse(loss, tag):
        pd_g = C.pde_desc(kind, dim, loss, ref["delta"], coef=GARBAGE)
        assert E.inverse_kernel_name(prog, pd_g, C.N) == q["inverse"]
        _poison(prog, pd_g, dev, nt, nx)
        flat = E.new_flat_grad(prog, dev)
        cg = torch.zeros(4, dtype=torch.float32, device=dev)
        r, s = E.residual_loss_grad_inverse(prog, pd_g, cv, x, t, scale, flat, cg, want_residual=True)
        _check_residual(tag, lane, r, s, ref, loss)
        _check_theta(tag, lane, prog, names, flat, ref[loss]["g"], TOL if loss == "mse" else 2 * TOL, floor(loss))
        _check_coef(tag, lane, cg.cpu(), ref[loss]["dc"])
        return r, s, flat, cg

    for loss in C.LOSSES:
        pd = C.pde_desc(kind, dim, loss, ref["delta"])
        gtol = TOL if loss == "mse" else 2 * TOL
        assert _lib.residual_unit_name(prog, pd, C.N) == q["unit"]
        # 1. forward only
        r1, s1 = E.residual_forward(prog, pd, x, t)
        _check_residual(f"{cid} {lane} {loss} forward", lane, r1, s1, ref, loss)
        # 2. fused residual + loss + gradient
        _poison(prog, pd, dev, nt, nx)
        flat = E.new_flat_grad(prog, dev)
        r2, s2 = E.residual_loss_grad(prog, pd, x, t, scale, flat, want_residual=True)
        _check_residual(f"{cid} {lane} {loss} fused", lane, r2, s2, ref, loss)
        _check_theta(f"{cid} {lane} {loss} fused", lane, prog, names, flat, ref[loss]["g"], gtol, floor(loss))
        # 4. inverse: coefficients from the device, their gradients from the same launch
        r4, _, _, _ = inverse(loss, f"{cid} {lane} {loss} inverse")
        # the 16-point family promises the same bits for a point's residual whichever call computes it
        # (csrc/jet_kernel_u16.h: forward-only and fused; csrc/pinn_abi.hip, use_merged: the inverse call of the merged units too)
        if fam in ("u16", "u16m"):
            assert torch.equal(r1, r2), f"{cid} {lane} {loss}: forward-only and fused residuals differ"
        if fam == "u16m":
            assert inv == "u16" and torch.equal(r2, r4), f"{cid} {lane} {loss}: fused and inverse residuals differ"
        if lane == "lm":  # the by-value coefficient path (pinn_residual_loss_grad_coef), layer-major only
            _poison(prog, pd, dev, nt, nx)
            flat = E.new_flat_grad(prog, dev)
            cg = torch.zeros(2, dtype=torch.float32, device=dev)
            r5, s5 = E.residual_loss_grad(prog, pd, x, t, scale, flat, want_residual=True, coef_grads=cg)
            tag = f"{cid} {lane} {loss} by-value"
            _check_residual(tag, lane, r5, s5, ref, loss)
            _check_theta(tag, lane, prog, names, flat, ref[loss]["g"], gtol, floor(loss))
            _check_coef(tag, lane, cg.cpu(), ref[loss]["dc"])

    # 3. the residual adjoint with a fixed cotangent (independent of the loss kind)
    pd = C.pde_desc(kind, dim)
    _poison(prog, pd, dev, nt, nx)
    flat = E.new_flat_grad(prog, dev)
    E.residual_backward(prog, pd, x, t, ref["rbar"].to(dev), flat)
    _check_theta(f"{cid} {lane} res_bar", lane, prog, names, flat, ref["gR"], TOL, floor("gR"))

    # the inverse call once more with the fixed-order reduction
    prog.set_deterministic(True)
    try:
        assert C.route(prog, kind, dim)["inverse"] == q["inverse"]
        inverse("mse", f"{cid} {lane} mse inverse deterministic")
    finally:
        prog.set_deterministic(False)
    _RAN.append((cid, lane, q["unit"], q["inverse"]))


def test_every_cell_ran_on_every_lane():
    """What ran is the table of tests/test_pde_epilogue_cpu.py (from the queries on descriptor-only programs)."""
    want = C.table()
    wall = time.time() - _T0
    summary = {"wall_s": wall, "ran": _RAN, "worst": _WORST, "widened": _WIDENED}
    print(json.dumps(summary, indent=1))
    try:
        out = os.environ.get("PINN_EPILOGUE_LOG", os.path.join(os.path.dirname(_PARITY_LOG), "parity_pde_epilogue.json"))  # beside the parity log
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1)
    except OSError:
        pass
    assert sorted(_RAN) == sorted(want), sorted(set(want) ^ set(_RAN))
    assert len(_RAN) == len(C.CASES)
