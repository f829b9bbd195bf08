"""GPU: every planned variant of the layer-major kernels against the fp64 oracle.

The layer-major engine (lm_engine.hip) launches lm_fused (30 translation units: 6 stream sets x 5 activation families,
24 variants each), lm_ew_fwd / lm_ew_bwd / lm_ew_bwd_dma, lm_fourier_fwd and lm_head (8 stream-set units here).  The
network list and the reachable matrix live in tests/lm_variants_model.py, tests/test_lm_variants_cpu.py proves without a
GPU that the list plans the whole matrix; here every network of the list runs, one case per (stream set, family), on
N = 100 points (three 32-point tiles and a ragged one), and `pinn_lm_plan` says which variants each launch takes: the
case asserts that the variants it exists for are planned, records them, and the last test checks that the recorded set
is the matrix of this process's policy.  tests/test_fused_policies.py reruns the module under PINN_LM_FUSED=0 and
PINN_LM_FUSED_LN=15.

Per network, against fp64 autograd through the oracle (`O.network_forward` with the composite LayerNorm,
`O.compute_residual`):
  (a) every jet stream separately;
  (b) the jet adjoint with a random cotangent, stream s scaled by 1 / |jet_s| — per tensor and concatenated;
  (c) residual, loss and gradient of residual_loss_grad, residual_forward bit-equal to it — per tensor and concatenated;
  (d) the residual adjoint with a random cotangent.
The cached workspace is filled with NaN before every reverse launch.

Bars: residual, loss, concatenated gradient 1e-5 (relu family, whose kinks may fall on the other side in fp32: 1e-4);
u and the derivative streams 2e-5, derivative streams of LayerNorm networks 5e-5; one state_dict tensor 1e-4.  A tensor
above 1e-4 is compared with the same oracle evaluated in fp32 on the CPU: if that floor against fp64 is itself above
2.5e-5 the tensor may take 4 x the floor (another summation order), otherwise the test fails; such tensors must stay
below 2 % of all compared tensors (last test).  Measured values: profiles/parity_lm_variants.md.
"""

import json
import os

import pytest
import torch

from conftest import _PARITY_LOG, rel_err, rel_l2
from hip_helpers import check_tensors
from test_wide_variants_gpu import PDE_OF, _cotangent, _grads, _params64, _pde_desc, _pde_spec, _points, _poison, _trainable

import lm_variants_model as M

pytestmark = pytest.mark.gpu

TOL = 1e-5
RELU_TOL = 1e-4
STREAM_TOL = 2e-5
LN_STREAM_TOL = 5e-5
WIDENED_CAP = 0.02  # TENSOR_TOL = 1e-4 and the fp32-floor rule: hip_helpers.check_tensors

POLICY = M.policy_of_env(os.environ)
RAN = set()
TENSORS = {"compared": 0, "widened": []}
WORST = {}  # (family, tensor kind) -> (value, where)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _has_ln(spec):
    return spec.architecture in ("resnet", "attention") or bool(spec.layer_norm)


def _jets_of(spec, params, x, t, nt, nx):
    import oracle as O

    x = x.clone().requires_grad_(True)
    t = t.clone().requires_grad_(True)
    u = O.network_forward(spec, params, torch.cat([x, t], 1), "composite")
    out, cur = [u], u
    for _ in range(nt):
        cur = torch.autograd.grad(cur, t, torch.ones_like(cur), create_graph=True)[0]
        out.append(cur)
    cur = u
    for _ in range(nx):
        cur = torch.autograd.grad(cur, x, torch.ones_like(cur), create_graph=True)[0][:, 0:1]
        out.append(cur)
    return out


def _oracle_eval(spec, pde_key, nt, nx, seed, n, dtype=torch.float64, like=None):
    """The oracle's results of one network in `dtype` (fp64: the reference; fp32: the floor of a tensor above its bar,
    with the cotangents of the fp64 evaluation `like`)."""
    import oracle as O

    sd = O.init_state_dict(spec, seed=seed)
    x, t = _points(spec.input_dim, n, seed + 1)
    cast = (lambda p: p) if dtype == torch.float64 else (lambda p: {k: v.detach().to(dtype).requires_grad_(v.requires_grad) for k, v in p.items()})
    params = cast(_params64(sd))
    names = _trainable(params)
    jets = _jets_of(spec, params, x.to(dtype), t.to(dtype), nt, nx)
    cot = like["cot"] if like else _cotangent(jets, seed + 2)
    adj = _grads(sum((cot[s].to(dtype) * jets[s].flatten()).sum() for s in range(len(jets))), params, names)
    res = {"sd": sd, "x": x, "t": t, "jets": [j.detach().flatten() for j in jets], "cot": cot, "adj": adj, "names": names}
    if pde_key is not None:
        pde = _pde_spec(*pde_key)
        params = cast(_params64(sd))
        r = O.compute_residual(pde, lambda inp: O.network_forward(spec, params, inp, "composite"), x.to(dtype), t.to(dtype))
        L = O.apply_loss_fn(r, pde.loss_function, pde.huber_delta)
        rbar = like["rbar"] if like else torch.randn(n, 1, generator=torch.Generator().manual_seed(seed + 3), dtype=torch.float64).float().double()
        res.update(pde=pde, r=r.detach(), L=L.detach(), rbar=rbar, gL=_grads(L, params, names, retain_graph=True),
                   gR=_grads((rbar.to(dtype) * r).sum(), params, names))
    return res


KINK_MARGIN = 2e-6


def _kink_margin(spec, sd, x, t):
    """Smallest |z| / rms(z over the layer's features) over every value a relu / leaky_relu of the network sees at these
    points, in fp64."""
    import oracle as O
    import torch.nn.functional as F

    seen = []
    orig = {"relu": F.relu, "leaky_relu": F.leaky_relu}

    def spy(name):
        def f(z, *a, **k):
            seen.append(float((z.abs() / z.pow(2).mean(-1, keepdim=True).sqrt()).min()))
            return orig[name](z, *a, **k)
        return f

    F.relu, F.leaky_relu = spy("relu"), spy("leaky_relu")
    try:
        with torch.no_grad():
            O.network_forward(spec, {k: v.double() for k, v in sd.items()}, torch.cat([x, t], 1).double(), "composite")
    finally:
        F.relu, F.leaky_relu = orig["relu"], orig["leaky_relu"]
    return min(seen)


def _seed_for(spec, seed, n):
    """The seed of a network.  The relu bar (1e-4) is for kinks that fp32 and fp64 place on the same side: the rounding
    error of a pre-activation z — a sum of up to 1 024 fp32 products, behind up to six layers — is a few 1e-7 of the rms of
    its layer, and a z closer to 0 than that may take the other branch in another summation order, which changes u_t and
    u_x at that point by the whole contribution of one feature (seen on the MI355X: 2.2e-3 on u_t with one z at 2.7e-7 of
    the rms, u itself at 2.9e-7).  So networks of the relu family take the first of seed, seed + 10 000, ... whose values in
    front of a relu all stay KINK_MARGIN = 2e-6 of their layer's rms away from 0; with ~160 000 such values in the widest
    network about three seeds in four qualify."""
    import oracle as O

    if spec.architecture == "siren" or spec.activation not in ("relu", "leaky_relu"):
        return seed
    for k in range(50):
        s = seed + 10000 * k
        x, t = _points(spec.input_dim, n, s + 1)
        if _kink_margin(spec, O.init_state_dict(spec, seed=s), x, t) >= KINK_MARGIN:
            return s
    raise AssertionError(f"no seed with every relu input {KINK_MARGIN:g} away from its kink: {spec}")


_SHAPES = {}


def _kind_of(spec, name):
    """Tensor kind for the profile: LayerNorm weight / bias; first, hidden and output Linear weight / bias."""
    import oracle as O

    sd = _SHAPES.setdefault(repr(spec), {k: v.dim() for k, v in O.init_state_dict(spec, seed=0).items()})
    part = "weight" if name.endswith("weight") else "bias"
    w = name[:-len(part)] + "weight"
    if sd[w] == 1:
        return "LayerNorm " + part
    linear = [k for k in sd if k.endswith("weight") and sd[k] == 2]
    return ("first" if w == linear[0] else ("output" if w == linear[-1] else "hidden")) + " Linear " + part


def _check_grads(prog, names_all, flat, want, what, tol, spec, fam, floor):
    """Per tensor and concatenated; `floor()` evaluates the fp32 oracle's gradients of the same quantity (lazily)."""
    from pinnrl_amd import engine as E

    by_name = {n: g for n, g in zip(names_all, E.split_flat_grad(prog, flat)) if g is not None}
    keys = [k for k in want if k in by_name]
    assert keys and len(keys) == len(want)
    got = torch.cat([by_name[k].flatten().cpu() for k in keys])
    assert torch.isfinite(got).all(), f"{what}: non-finite gradient"

    def seen(k, e):
        TENSORS["compared"] += 1
        kind = (fam, _kind_of(spec, k))
        if e > WORST.get(kind, (0.0, ""))[0]:
            WORST[kind] = (e, f"{what} {k}")
        print(f"{what}: tensor {k}: {e:.2e}")

    TENSORS["widened"] += check_tensors(by_name, want, what, floor, seen)
    e = rel_l2(got, torch.cat([want[k].flatten() for k in keys]), label=f"{what} gradient", tol=tol)
    print(f"{what}: concatenated gradient {e:.2e}")
    assert e <= tol, f"{what}: concatenated gradient {e:.2e}"


def _run_network(dev, nt, nx, fam, label, spec, seed, n=M.N_PTS):
    from hip_helpers import program_from_spec
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    K = 1 + nt + nx
    pde_key = PDE_OF[(nt, nx)]
    tag = f"({nt},{nx}) {fam} {label}"
    fwd_variants, bwd_variants = M.network_variants(label, spec, nt, nx, fam, POLICY, n)  # asserts the case's subject is planned
    seed = _seed_for(spec, seed, n)
    o = _oracle_eval(spec, pde_key, nt, nx, seed, n)
    floors = {}

    def floor(which):
        def get():
            if "o32" not in floors:
                floors["o32"] = _oracle_eval(spec, pde_key, nt, nx, seed, n, torch.float32, like=o)
            return floors["o32"][which]
        return get

    prog, names_all = program_from_spec(spec, o["sd"], dev)
    prog.set_layer_major(True)
    assert _lib.kernel_for(prog, n, nt, nx, 1)["engine"] == "layer_major", tag
    relu = spec.activation in ("relu", "leaky_relu") and spec.architecture != "siren"
    tol = RELU_TOL if relu else TOL
    u_tol = RELU_TOL if relu else STREAM_TOL
    jet_tol = RELU_TOL if relu else (LN_STREAM_TOL if _has_ln(spec) else STREAM_TOL)
    x, t = o["x"].to(dev), o["t"].to(dev)
    # (a) every stream of the forward launch
    jets = E.jets_forward(prog, x, t, nt, nx).cpu()
    for s in range(K):
        w = o["jets"][s]
        if float(w.norm()) == 0.0:  # relu without LayerNorm: second derivatives vanish identically
            assert float(jets[s].abs().max()) == 0.0, (tag, s)
            continue
        bar = u_tol if s == 0 else jet_tol
        e = rel_l2(jets[s], w, label=f"{tag} jet stream {s}", tol=bar)
        print(f"{tag}: jet stream {s}: {e:.2e}")
        assert e <= bar, f"{tag}: jet stream {s}: {e:.2e}"
    # (b) jet adjoint
    _poison(prog, dev, n, nt, nx)
    flat = E.new_flat_grad(prog, dev)
    E.jets_backward(prog, x, t, nt, nx, o["cot"].float().to(dev), flat)
    _check_grads(prog, names_all, flat, o["adj"], f"{tag} adjoint", tol, spec, fam, floor("adj"))
    if pde_key is not None:
        pd = _pde_desc(o["pde"])
        # (c) residual + loss + gradient; the forward-only launch gives the same bits
        _poison(prog, dev, n, nt, nx)
        flat = E.new_flat_grad(prog, dev)
        r, s = E.residual_loss_grad(prog, pd, x, t, 1.0 / n, flat, want_residual=True)
        e = rel_l2(r.cpu(), o["r"], label=f"{tag} residual", tol=tol)
        print(f"{tag}: residual {e:.2e}")
        assert e <= tol, f"{tag}: residual {e:.2e}"
        e = rel_err(float(s) / n, float(o["L"]), label=f"{tag} loss", tol=tol)
        assert e <= tol, f"{tag}: loss {e:.2e}"
        _check_grads(prog, names_all, flat, o["gL"], f"{tag} loss", tol, spec, fam, floor("gL"))
        r0, s0 = E.residual_forward(prog, pd, x, t)
        assert torch.equal(r0, r), f"{tag}: residual_forward and residual_loss_grad differ"
        assert rel_err(float(s0) / n, float(o["L"]), label=f"{tag} forward loss", tol=tol) <= tol, tag
        # (d) residual adjoint
        _poison(prog, dev, n, nt, nx)
        flat = E.new_flat_grad(prog, dev)
        E.residual_backward(prog, pd, x, t, o["rbar"].float().to(dev), flat)
        _check_grads(prog, names_all, flat, o["gR"], f"{tag} residual adjoint", tol, spec, fam, floor("gR"))
    RAN.update(fwd_variants | bwd_variants)


@pytest.mark.parametrize("nt,nx,fam", M.cases(), ids=lambda v: str(v))
def test_case_variants(nt, nx, fam, dev):
    """One (stream set, family) case: its networks, forward and reverse, every check of the module docstring."""
    for j, (label, spec) in enumerate(M.networks(nt, nx, fam)):
        _run_network(dev, nt, nx, fam, label, spec, seed=3000 + 100 * M.SETS.index((nt, nx)) + 10 * M.FAMILIES.index(fam) + j)


def test_matrix_is_complete():
    """Runs after the matrix (file order): the recorded variants are the reachable matrix of this process's policy, and
    the tensors on a widened bar stay below 2 % of all compared tensors."""
    full = M.reachable(POLICY)
    n_w, n_c = len(TENSORS["widened"]), TENSORS["compared"]
    print(f"layer-major variant matrix ({POLICY}): {len(RAN & full)} of {len(full)} variants ran; {n_w} of {n_c} tensors on a widened bar")
    summary = {"policy": POLICY, "ran": len(RAN & full), "reachable": len(full), "tensors_compared": n_c, "widened": TENSORS["widened"],
               "worst": {f"{f} | {k}": {"value": v, "where": w} for (f, k), (v, w) in sorted(WORST.items())}}
    try:  # next to the log of every measured error (conftest._PARITY_LOG): what profiles/parity_lm_variants.md is made from
        out_dir = os.path.dirname(_PARITY_LOG)
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"lm_variants_{POLICY}.json"), "w") as fh:
            json.dump(summary, fh, indent=1)
    except OSError:
        pass
    assert RAN == full, f"variants that did not run: {sorted(full - RAN)[:20]}; outside the matrix: {sorted(RAN - full)[:20]}"
    assert n_c > 0 and n_w < WIDENED_CAP * n_c, TENSORS["widened"]
