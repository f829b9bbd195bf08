"""CPU tests (no GPU) of coupled systems: `pinn_term_residual_system`, component launches, `TermPDESystem`.

(a) the fp64 model of tests/term_system_model.py against fp64 autograd of the written-out formulas of Gray-Scott 1-D and
    Navier-Stokes 2-D (nested autograd of analytic fields supplies the jets), to 1e-12; the Navier-Stokes program on the
    analytic Taylor-Green fields and their analytic derivatives: residuals <= 1e-12; the seeds of the kernel test keep the
    kinks of the loss clear;
(b) header, `_lib.EXPORTS` and the library agree, still ABI 2;
(c) every host-side rejection of the entry point, with made-up addresses and no device;
(d) `engine.NetProgram` of a multi-output network, `engine.SystemTermDesc`;
(e) `TermPDESystem`: the orders it derives, its constructor refusals, the trainer's routing and refusals.
"""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import pinnrl_amd.pdes as P
import term_system_model as M
from pinnrl_amd import _lib
from pinnrl_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
f64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model
# ---------------------------------------------------------------------------------------------------------------------
def _d(f, v, k):
    """k-th derivative of f (a tensor built from v) with respect to v, by nested autograd."""
    for _ in range(k):
        f, = torch.autograd.grad(f.sum(), v, create_graph=True)
    return f


def _analytic_jets(fields, dim, nt, nx, x, t):
    """The 3 C blocks of the given analytic fields (functions of the coordinate columns and t) by nested fp64 autograd."""
    cols = [x[:, a].clone().requires_grad_(True) for a in range(dim)]
    tt = t.clone().requires_grad_(True)
    jets = []
    for c, fn in enumerate(fields):
        u = fn(*cols, tt)
        rows = [u] + [_d(u, tt, k) for k in range(1, nt[c] + 1)] + [_d(u, cols[0], k) for k in range(1, nx[c][0] + 1)]
        jets.append(torch.stack(rows).detach())
        for a in (1, 2):
            if a < dim and nx[c][a] > 0:
                jets.append(torch.stack([u] + [_d(u, cols[a], k) for k in range(1, nx[c][a] + 1)]).detach())
            else:
                jets.append(None)
    return jets


def _loss_sum(r, loss, delta):
    if loss == "mae":
        return r.abs().sum()
    if loss == "huber":
        a = r.abs()
        return torch.where(a < delta, 0.5 * r * r, delta * (a - 0.5 * delta)).sum()
    return (r * r).sum()


def _gray_scott_formula(j, coef):
    """The two Gray-Scott residuals written out on the blocks [u | - | - | v | - | -], rows [u, u_t, u_x, u_xx]."""
    U, V = j[0], j[3]
    u, v = U[0], V[0]
    r0 = coef[0] * U[1] + coef[1] * U[3] + coef[2] * u * v * v + coef[3] + coef[4] * u
    r1 = coef[5] * V[1] + coef[6] * V[3] + coef[7] * u * v * v + coef[8] * v
    return torch.stack([r0, r1])


def _navier_stokes_formula(j, coef):
    """Momentum in x and y and continuity on the blocks of (u, v, p): axis-0 rows [f, f_t, f_x, f_xx] ([p, p_t, p_x] for the
    pressure), axis-1 rows [f, f_y, f_yy] ([p, p_y])."""
    U, Uy, V, Vy, Pr, Py = j[0], j[1], j[3], j[4], j[6], j[7]
    u, v = U[0], V[0]
    r0 = coef[0] * U[1] + coef[1] * u * U[2] + coef[2] * v * Uy[1] + coef[3] * Pr[2] + coef[4] * U[3] + coef[5] * Uy[2]
    r1 = coef[6] * V[1] + coef[7] * u * V[2] + coef[8] * v * Vy[1] + coef[9] * Py[1] + coef[10] * V[3] + coef[11] * Vy[2]
    r2 = coef[12] * U[2] + coef[13] * Vy[1]
    return torch.stack([r0, r1, r2])


_FORMULA = {"gray_scott": _gray_scott_formula, "navier_stokes": _navier_stokes_formula}
_FIELDS = {
    "gray_scott": [lambda x, t: 1.0 - 0.5 * torch.exp(-3.0 * x * x) * torch.cos(t), lambda x, t: 0.25 * torch.exp(-2.0 * x * x) + 0.1 * torch.sin(x + t)],
    "navier_stokes": [lambda x, y, t: torch.sin(x + 0.5 * y) * torch.exp(-t) + 0.2 * x * y,
                      lambda x, y, t: torch.cos(x * y) + 0.3 * t * torch.sin(y),
                      lambda x, y, t: torch.sin(x) * torch.cos(y) * (1.0 + t)],
}


@pytest.mark.parametrize("loss,delta", M.LOSSES)
@pytest.mark.parametrize("name", ["gray_scott", "navier_stokes"])
def test_model_matches_autograd_of_the_written_out_formulas(name, loss, delta):
    dim, nt, nx, n_eq, terms, coef = M.PROGRAMS[name]
    w = M.EQ_WEIGHTS[name]
    N, gs = 40, 0.37
    g = torch.Generator().manual_seed(1)
    x = torch.rand(N, dim, generator=g, dtype=f64) * 2 - 1
    t = torch.rand(N, generator=g, dtype=f64)
    jets = _analytic_jets(_FIELDS[name], dim, nt, nx, x, t)
    leaves = [None if j is None else j.clone().requires_grad_(True) for j in jets]
    c64 = torch.tensor(coef, dtype=f64, requires_grad=True)
    r = _FORMULA[name](leaves, c64)
    per_eq = torch.stack([_loss_sum(r[e], loss, delta) for e in range(n_eq)])
    total = gs * (torch.tensor(w, dtype=f64) * per_eq).sum()
    live = [j for j in leaves if j is not None]
    grads = torch.autograd.grad(total, live + [c64])
    m = M.evaluate(dim, nt, nx, n_eq, terms, coef, [None if j is None else j.numpy() for j in jets], x.numpy(), t.numpy(), w, loss,
                   delta, gs)
    assert np.max(np.abs(m["r"] - r.detach().numpy())) <= 1e-12
    assert np.max(np.abs(m["eq_loss"] - per_eq.detach().numpy())) <= 1e-12 * max(1.0, float(per_eq.detach().abs().max()))
    assert abs(m["loss_sum"] - float((torch.tensor(w, dtype=f64) * per_eq.detach()).sum())) <= 1e-12 * max(1.0, m["loss_abs"])
    it = iter(grads[:-1])
    for b, j in enumerate(leaves):
        if j is None:
            assert m["cot"][b] is None
            continue
        want = next(it).numpy().copy()
        if b % 3:
            assert not np.any(want[0])  # the formulas take the value from block (c, 0) alone
        assert np.max(np.abs(m["cot"][b] - want)) <= 1e-12, (name, b)
        for row in range(want.shape[0]):
            assert m["touched"][b][row] or not np.any(m["cot"][b][row])
    assert np.max(np.abs(m["coef_sums"] - grads[-1].numpy())) <= 1e-12 * max(1.0, float(np.max(m["coef_abs"])))
    # a given (E, N) cotangent: the vector-Jacobian product of the residual field
    rbar = torch.randn(n_eq, N, generator=g, dtype=f64)
    grads = torch.autograd.grad((rbar * _FORMULA[name](leaves, c64)).sum(), live)
    m = M.evaluate(dim, nt, nx, n_eq, terms, coef, [None if j is None else j.numpy() for j in jets], x.numpy(), t.numpy(), w, loss,
                   delta, gs, residual_cotangent=rbar.numpy())
    for want, got in zip(grads, [c for c in m["cot"] if c is not None]):
        assert np.max(np.abs(got - want.numpy())) <= 1e-12


def test_navier_stokes_program_vanishes_on_taylor_green():
    """u = -cos x sin y F, v = sin x cos y F, p = -(cos 2x + cos 2y) F^2 / 4, F = exp(-2 nu t): analytic derivatives in, zero out."""
    nu = 0.1
    dim, nt, nx, n_eq, terms, coef = M.PROGRAMS["navier_stokes"]
    assert coef[4] == -nu
    rng = np.random.default_rng(3)
    N = 64
    x, y, t = rng.uniform(-3, 3, N), rng.uniform(-3, 3, N), rng.uniform(0, 1, N)
    F = np.exp(-2 * nu * t)
    s, c = np.sin, np.cos
    u, v = -c(x) * s(y) * F, s(x) * c(y) * F
    jets = [
        np.stack([u, -2 * nu * u, s(x) * s(y) * F, -u]), np.stack([u, -c(x) * c(y) * F, -u]), None,
        np.stack([v, -2 * nu * v, c(x) * c(y) * F, -v]), np.stack([v, -s(x) * s(y) * F, -v]), None,
        np.stack([-(c(2 * x) + c(2 * y)) * F * F / 4, nu * (c(2 * x) + c(2 * y)) * F * F, s(2 * x) * F * F / 2]),
        np.stack([-(c(2 * x) + c(2 * y)) * F * F / 4, s(2 * y) * F * F / 2]), None,
    ]
    m = M.evaluate(dim, nt, nx, n_eq, terms, coef, jets, np.stack([x, y], 1), t)
    assert np.max(np.abs(m["r"])) <= 1e-12


@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_seeds_keep_the_kinks_of_the_loss_clear(name):
    for N in M.SIZES[:-1]:
        dim, nt, nx, n_eq, terms, coef, jets, x, t, rbar = M.inputs(name, N)
        for loss, delta in M.LOSSES:
            m = M.evaluate(dim, nt, nx, n_eq, terms, coef, jets, x, t, M.EQ_WEIGHTS[name], loss, delta, 1.0 / N)
            assert m["unsafe"].any(0).sum() <= 0.01 * N, (name, N, loss)


def test_programs_cover_what_the_issue_names():
    gs, ns, caps, un = (M.PROGRAMS[k] for k in ("gray_scott", "navier_stokes", "caps", "unnamed_field"))
    assert len(gs[1]) == gs[3] == 2 and any(f == () for _, f in gs[4]) and any(f == ((0, "u"), (1, "u"), (1, "u")) for _, f in gs[4])
    assert len(ns[1]) == ns[3] == 3 and len(ns[4]) == 14 and ns[0] == 2
    assert len(caps[1]) == caps[3] == 4 and len(caps[4]) == 32 and caps[0] == 3 and all(len(f) == 4 for _, f in caps[4])
    flat = [f for _, fs in caps[4] for f in fs]
    assert any(f in ("x", "y", "z", "t") for f in flat) and any(not isinstance(f, str) and f[1] in ("sin(u)", "cos(u)") for f in flat)
    assert not any(not isinstance(f, str) and f[0] == 1 for _, fs in un[4] for f in fs) and len(un[1]) == 3


# ---------------------------------------------------------------------------------------------------------------------
# (b) header, binding, library
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pinn_jet.h")).read()
    assert re.search(r"\bint pinn_term_residual_system\s*\(", hdr)
    assert "pinn_term_residual_system" in _lib.EXPORTS and hasattr(_lib.load(), "pinn_term_residual_system")
    assert _lib.load().pinn_abi_version() == 2 == _lib.PINN_ABI_VERSION and re.search(r"#define PINN_ABI_VERSION 2\b", hdr)
    for name, value in (("MAX_FIELDS", 4), ("MAX_EQUATIONS", 4), ("MAX_TERMS", 32)):
        assert re.search(rf"#define PINN_SYSTEM_{name} {value}\b", hdr) and getattr(_lib, f"PINN_SYSTEM_{name}") == value
    assert re.search(r"#define PINN_SYSTEM_SCRATCH_DOUBLES \(64 \* \(4 \+ 32\)\)", hdr) and _lib.PINN_SYSTEM_SCRATCH_DOUBLES == 64 * 36
    assert _lib.PINN_SYSTEM_FACTOR(3, 16) == 112 and _lib.PINN_SYSTEM_FACTOR(0, 0) == 0
    assert ctypes.sizeof(_lib.PinnTermPdeSystem) == 4 * (3 + 4 + 12 + 1 + 32 + 4 + 2 + 32 * 5)
    assert ctypes.sizeof(_lib.PinnTermPdeAxes) == 4 * (8 + 16 * 5) and _lib.PINN_TERM_MAX_TERMS == 16  # the siblings are untouched
    assert "Components of a multi-output network" in hdr and "PINN_FLAG_LAYER_MAJOR is required whenever row k is not 16-byte aligned" in hdr


# ---------------------------------------------------------------------------------------------------------------------
# (c) host-side validation
# ---------------------------------------------------------------------------------------------------------------------
def _desc(dim=2, C=2, E_=2, nt=(1, 1), nx=((2, 2, 0), (1, 1, 0)), terms=((0, ((0, 1),)), (1, ((1, 3), (0, 11)))), w=(1.0, 1.0)):
    """A raw descriptor: terms = ((equation, ((field, code), ...)), ...)."""
    d = _lib.PinnTermPdeSystem()
    d.dimension, d.n_fields, d.n_equations, d.n_terms = dim, C, E_, len(terms)
    for c in range(min(C, len(nt))):
        d.time_order[c] = nt[c]
        for a in range(3):
            d.space_order[c][a] = nx[c][a]
    for e in range(min(E_, len(w))):
        d.eq_weight[e] = w[e]
    d.loss, d.huber_delta = 0, 1.0
    for m, (e, factors) in enumerate(terms[:32]):
        d.equation_of[m] = e
        d.terms[m].n_factors = len(factors)
        for f, (field, code) in enumerate(factors[:4]):
            d.terms[m].factor[f] = field * 32 + code
    return d


def _table(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _default_table(d):
    out = []
    for c in range(max(0, min(d.n_fields, 4))):
        out += [0x1000 * (3 * c + 1), 0x1000 * (3 * c + 2) if d.space_order[c][1] else None, 0x1000 * (3 * c + 3) if d.space_order[c][2] else None]
    return _table(*out)


def _call(d, coef=0x1000, jets="default", x=0x1000, t=0x1000, N=8, scratch=None, loss_sum=None, eq=None, cot=None, cg=None):
    lib = _lib.load()
    if jets == "default":
        jets = _default_table(d)
    return lib.pinn_term_residual_system(ctypes.byref(d), coef, jets, x, t, N, 1.0, None, None, loss_sum, eq, cot, cg, scratch, None)


def test_term_residual_system_validation_is_answered_on_the_host():
    """Every rejection comes back before any HIP call: the addresses are made up and there is no device."""
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pinn_jet.h")).read()
    BAD = int(re.search(r"PINN_ERR_BAD_DESC\s*=\s*(-?\d+)", hdr).group(1))
    MIS = int(re.search(r"PINN_ERR_MISALIGNED\s*=\s*(-?\d+)", hdr).group(1))
    err = lambda: lib.pinn_last_error().decode()  # noqa: E731
    assert lib.pinn_term_residual_system(None, 0x1000, _table(0x1000), None, None, 8, 1.0, None, None, None, None, None, None, None, None) == BAD
    # ranges
    for dim in (0, 4):
        assert _call(_desc(dim=dim)) == BAD and "dimension" in err()
    for C in (0, 5):
        assert _call(_desc(C=C)) == BAD and "n_fields" in err()
    for n in (0, 5):
        assert _call(_desc(E_=n)) == BAD and "n_equations" in err()
    d = _desc()
    d.n_terms = 33
    assert _call(d) == BAD and "n_terms" in err()
    d.n_terms = -1
    assert _call(d) == BAD and "n_terms" in err()
    d = _desc()
    d.terms[0].n_factors = 5
    assert _call(d) == BAD and "n_factors" in err()
    # stream sets and orders
    assert _call(_desc(nt=(1, 0), nx=((2, 2, 0), (1, 1, 0)))) == BAD and "field 1" in err() and "not compiled" in err()  # (0, 1) on axis 0
    assert _call(_desc(nt=(2, 1), nx=((1, 0, 0), (1, 1, 0)), terms=())) == BAD and "not compiled" in err()
    assert _call(_desc(nx=((2, 3, 0), (1, 1, 0)))) == BAD and "space_order[1]" in err()
    assert _call(_desc(nx=((2, 2, 1), (1, 1, 0)))) == BAD and "space_order[2]" in err()  # beyond dimension 2
    assert _call(_desc(dim=1, nx=((2, 1, 0), (1, 0, 0)), terms=())) == BAD and "space_order[1]" in err()
    assert _call(_desc(nx=((2, -1, 0), (1, 1, 0)))) == BAD
    # equations and weights
    assert _call(_desc(terms=((2, ((0, 1),)),))) == BAD and "equation_of[0]" in err()
    assert _call(_desc(terms=((-1, ((0, 1),)),))) == BAD and "equation_of[0]" in err()
    for bad_w in (-1.0, float("nan"), float("inf")):
        assert _call(_desc(w=(1.0, bad_w))) == BAD and "eq_weight[1]" in err()
    # factors
    assert _call(_desc(terms=((0, ((0, 17),)),))) == BAD and "unknown factor code" in err()   # a mixed-derivative code
    assert _call(_desc(terms=((0, ((0, 31),)),))) == BAD and "unknown factor code" in err()
    d = _desc()
    d.terms[0].factor[0] = 256
    assert _call(d) == BAD and "one byte" in err()
    d.terms[0].factor[0] = -1
    assert _call(d) == BAD and "one byte" in err()
    assert _call(_desc(terms=((0, ((2, 0),)),))) == BAD and "field 2 of 2" in err()
    assert _call(_desc(terms=((0, ((0, 2),)),))) == BAD and "does not hold" in err()    # u_tt with nt = 1
    assert _call(_desc(terms=((0, ((1, 4),)),))) == BAD and "does not hold" in err()    # v_xx with nx0 = 1
    assert _call(_desc(terms=((0, ((1, 12),)),))) == BAD and "does not hold" in err()   # v_yy with nx1 = 1
    assert _call(_desc(terms=((0, ((0, 13),)),))) == BAD and "does not hold" in err()   # u_z in dimension 2
    assert _call(_desc(terms=((0, ((0, 16),)),))) == BAD and "coordinate" in err()      # z in dimension 2
    assert _call(_desc(dim=1, nx=((2, 0, 0), (1, 0, 0)), terms=((0, ((0, 15),)),))) == BAD and "coordinate" in err()  # y in 1-D
    # N and the tables
    assert _call(_desc(), N=-1) == BAD and "N < 0" in err()
    assert _call(_desc(), N=0, jets=None, coef=None) == 0                               # N == 0 is a no-op
    assert _call(_desc(), jets=None) == BAD and "null jets table" in err()
    assert _call(_desc(), coef=None) == BAD and "coef_values" in err()
    good = _default_table(_desc())
    for b in (0, 1, 3, 4):
        tab = _table(*[None if i == b else good[i] for i in range(6)])
        assert _call(_desc(), jets=tab) == BAD and f"(field {b // 3}, axis {b % 3})" in err()
        assert _call(_desc(), cot=tab) == BAD and f"(field {b // 3}, axis {b % 3})" in err()
    assert _call(_desc(terms=((0, ((0, 7),)),)), x=None) == BAD and "coordinate array is null" in err()
    assert _call(_desc(terms=((0, ((3, 15),)),)), x=None) == BAD and "coordinate array is null" in err()  # field bits ignored
    assert _call(_desc(terms=((0, ((0, 8),)),)), t=None) == BAD and "coordinate array is null" in err()
    for kw in ("loss_sum", "eq", "cg"):
        assert _call(_desc(), **{kw: 0x1000}) == BAD and "scratch" in err()
        assert _call(_desc(), scratch=0x1004, **{kw: 0x1000}) == MIS and "8-byte" in err()


# ---------------------------------------------------------------------------------------------------------------------
# (d) the engine objects
# ---------------------------------------------------------------------------------------------------------------------
def _program(C=3, H=30, din=3, ln=False):
    tensors = [torch.zeros(H, din), torch.zeros(H)] + ([torch.ones(H), torch.zeros(H)] if ln else [])
    tensors += [torch.zeros(H, H), torch.zeros(H)] + ([torch.ones(H), torch.zeros(H)] if ln else []) + [torch.zeros(C, H), torch.zeros(C)]
    return E.NetProgram("feedforward", "tanh", din, [H, H, C], tensors, [True] * len(tensors), layer_norm=ln)


def test_net_program_of_a_multi_output_network():
    prog = _program()
    d = prog.desc
    assert prog.n_outputs == 3 and d.num_linear == 3 and [d.widths[i] for i in range(3)] == [30, 30, 1]
    assert [prog.component_offsets(k) for k in range(3)] == [(0, 0), (30, 1), (60, 2)]
    base, k = prog._weight_ptrs(), 2
    ptrs = prog._weight_ptrs(k)
    assert [ptrs[i] for i in range(4)] == [base[i] for i in range(4)]
    assert ptrs[4] == base[4] + 4 * 60 and ptrs[5] == base[5] + 4 * 2 
    assert (prog._weight_ptrs(1)[4] - base[4]) % 16 == 8  # row 1 of width 30 is not 16-byte aligned
    offs, n = prog.grad_layout()
    assert offs == [0, 92, 124, 1024, 1056, 1148] and n == 1152  # unchanged rule; the output weight's slot holds C H = 90 floats
    flat = torch.zeros(n)
    gbase, g = E._grad_ptrs(prog, flat), E._grad_ptrs(prog, flat, k)
    assert g[4] == gbase[4] + 4 * 60 and g[5] == gbase[5] + 4 * 2 and [g[i] for i in range(4)] == [gbase[i] for i in range(4)]
    assert E.split_flat_grad(prog, flat)[4].shape == (3, 30)
    # routing: a by-value copy with PINN_FLAG_LAYER_MAJOR, composed with the axis and direction bits; the program's own stays
    for kw, bits in ((dict(), 0), (dict(axis=1), 0x100), (dict(direction=(1, 1)), 0x1400)):
        dd = E._launch_desc(prog, component=1, **kw)
        assert dd is not d and dd.flags == _lib.PINN_FLAG_LAYER_MAJOR | bits and d.flags == 0 and dd.widths[2] == 1
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    dd = E._launch_desc(prog, component=1)
    assert lib.pinn_kernel_name(ctypes.byref(dd), 100, 1, 2, 1, buf, 64) == 0 and buf.value == b"layer_major"
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="component"):
            E._launch_desc(prog, component=bad)
    with pytest.raises(NotImplementedError, match="1 to 4"):
        _program(C=5)
    one = _program(C=1, H=32)
    assert one.n_outputs == 1 and E._launch_desc(one) is one.desc and one.desc.flags == 0
    with pytest.raises(ValueError, match="component"):
        E._launch_desc(one, component=1)
    with pytest.raises(NotImplementedError, match="one output"):
        E._single_output(prog, "a compiled residual")


def test_system_term_desc():
    dim, nt, nx, n_eq, terms, coef = M.PROGRAMS["navier_stokes"]
    factors, eq_of = M.engine_terms(terms)
    cv = torch.tensor(coef)
    td = E.SystemTermDesc(factors, eq_of, cv, dim, 3, n_eq, nt, nx, (1.0, 1.0, 4.0), "huber", 0.5)
    d = td.desc
    assert (d.dimension, d.n_fields, d.n_equations, d.n_terms, d.loss) == (2, 3, 3, 14, _lib.LOSS["huber"])
    assert [d.equation_of[m] for m in range(14)] == eq_of and [d.eq_weight[e] for e in range(3)] == [1.0, 1.0, 4.0]
    assert d.terms[2].n_factors == 2 and [d.terms[2].factor[f] for f in range(2)] == [32 + 0, 0 + 11]  # v u_y
    assert d.terms[3].factor[0] == 64 + 3                                                               # p_x
    assert td.launches() == [(0, 0, 1, 2), (0, 1, 0, 2), (1, 0, 1, 2), (1, 1, 0, 2), (2, 0, 1, 1), (2, 1, 0, 1)]
    assert E.pde_streams(td) == (1, 2)
    td2 = td.with_loss("mae")
    assert td2.desc.loss == _lib.LOSS["mae"] and td2.coef_values is cv and td2.terms == td.terms
    tdc = E.SystemTermDesc([("x", (1, "u"))], [0], cv, 2, 2, 1, (0, 0), ((0, 0, 0), (0, 0, 0)))
    assert [tdc.desc.terms[0].factor[f] for f in range(2)] == [7, 32]
    for kw, msg in ((dict(dimension=4), "dimension"), (dict(n_fields=5), "fields"), (dict(n_equations=0), "equations"),
                    (dict(equation_of=[3] + eq_of[1:]), "equation_of"), (dict(eq_weights=(1.0, -1.0, 1.0)), "eq_weights"),
                    (dict(nx=((2, 3, 0), (2, 2, 0), (1, 1, 0))), "space orders")):
        args = dict(terms=factors, equation_of=eq_of, coef_values=cv, dimension=dim, n_fields=3, n_equations=n_eq, nt=nt, nx=nx)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            E.SystemTermDesc(**args)
    with pytest.raises(ValueError, match="unknown factor 'u_xy'.*mixed derivatives"):
        E.SystemTermDesc([((0, "u_xy"),)], [0], cv, 2, 1, 1, (1,), ((2, 2, 0),))
    with pytest.raises(ValueError, match="needs its field"):
        E.SystemTermDesc([("u_t",)], [0], cv, 2, 1, 1, (1,), ((2, 2, 0),))
    with pytest.raises(ValueError, match="names field 2 of 2"):
        E.SystemTermDesc([((2, "u"),)], [0], cv, 2, 2, 1, (1, 1), ((2, 2, 0), (2, 2, 0)))
    with pytest.raises(ValueError, match="at most 32 terms"):
        E.SystemTermDesc([()] * 33, [0] * 33, torch.zeros(33), 1, 1, 1, (0,), ((0, 0, 0),))
    with pytest.raises(RuntimeError, match="ROCm device"):
        E.term_residual_system(td, [torch.zeros(4, 8)] + [None] * 8, torch.zeros(8, 2), torch.zeros(8))


# ---------------------------------------------------------------------------------------------------------------------
# (e) TermPDESystem
# ---------------------------------------------------------------------------------------------------------------------
GRAY_SCOTT = [[(1.0, ("u_t",)), ((-1.0, "Du"), ("u_xx",)), (1.0, ("u", "v", "v")), ((-1.0, "F"), ()), ((1.0, "F"), ("u",))],
              [(1.0, ("v_t",)), ((-1.0, "Dv"), ("v_xx",)), (-1.0, ("u", "v", "v")), ((1.0, "Fk"), ("v",))]]
NAVIER_STOKES = [
    [(1.0, ("u_t",)), (1.0, ("u", "u_x")), (1.0, ("v", "u_y")), (1.0, ("p_x",)), ((-1.0, "nu"), ("u_xx",)), ((-1.0, "nu"), ("u_yy",))],
    [(1.0, ("v_t",)), (1.0, ("u", "v_x")), (1.0, ("v", "v_y")), (1.0, ("p_y",)), ((-1.0, "nu"), ("v_xx",)), ((-1.0, "nu"), ("v_yy",))],
    [(1.0, ("u_x",)), (1.0, ("v_y",))]]


def _config(dimension=1, bcs=None, **kw):
    return P.PDEConfig(
        name="system", domain=[(-1.0, 1.0), (0.0, 1.0), (0.0, 2.0)][:dimension], time_domain=(0.0, 0.5),
        parameters={"Du": 0.16, "Dv": 0.08, "F": 0.035, "Fk": 0.1, "nu": 0.1},
        boundary_conditions=bcs if bcs is not None else {"periodic": {}}, initial_condition={}, exact_solution={}, dimension=dimension,
        device=CPU, **kw)


def _ic2(x):
    return torch.stack([1 - 0.5 * torch.exp(-50 * x[:, 0] ** 2), 0.25 * torch.exp(-50 * x[:, 0] ** 2)], 1)


def test_what_term_pde_system_derives():
    cfg = _config()
    pde = P.TermPDESystem(cfg, ("u", "v"), GRAY_SCOTT, _ic2)
    assert cfg.output_dim == 2 and pde.n_fields == 2 and pde.n_equations == 2 and isinstance(pde, P.PDEBase)
    assert (pde._nt, pde._nx) == ((1, 1), ((2, 0, 0), (2, 0, 0))) and pde._equation_of == [0] * 5 + [1] * 4
    td = pde._pde_desc()
    assert isinstance(td, E.SystemTermDesc) and td is pde._pde_desc() and td.coef_values is pde.coef_values
    assert td.coef_values.tolist() == pytest.approx([1.0, -0.16, 1.0, -0.035, 0.035, 1.0, -0.08, -1.0, 0.1])
    assert td.terms[2] == ((0, "u"), (1, "u"), (1, "u")) and td.terms[3] == () and td.launches() == [(0, 0, 1, 2), (1, 0, 1, 2)]
    assert pde._pde_desc_l1().desc.loss == _lib.LOSS["mae"]
    ch = pde._manual_chain(100)  # 1-D: the two ends times the time grid, the line at t0
    assert ch["components"] == 2 and ch["x"].shape == (2 * 16 + 32, 1) and ch["n_bc"] == 2 and (ch["nt"], ch["nx"]) == (0, 0)
    assert [(lo, hi, st, pr) for lo, hi, st, pr, _, _ in ch["terms"]] == [(0, 16, 0, 16), (0, 16, 1, 16), (32, 64, 0, 0), (32, 64, 1, 0)]
    assert torch.equal(ch["x"][:16], torch.full((16, 1), -1.0)) and torch.equal(ch["x"][16:32], torch.full((16, 1), 1.0))
    assert torch.equal(ch["t"][:16], ch["t"][16:32]) and float(ch["t"][32:].abs().max()) == 0.0
    assert torch.equal(ch["terms"][3][4], _ic2(ch["x"][32:])[:, 1])
    # Navier-Stokes 2-D: the pressure has no boundary and no initial term; its set is (1, 1)
    ns = P.TermPDESystem(_config(2, {"dirichlet": {"type": "fixed", "value": [0.0, 0.5, None]}}), ("u", "v", "p"), NAVIER_STOKES,
                         lambda x: torch.stack([torch.sin(x[:, 0]), torch.cos(x[:, 1])], 1), initial_condition_fields=("u", "v"),
                         equation_weights=(1.0, 1.0, 4.0), boundary_points_per_axis=4, initial_points_per_axis=5)
    assert (ns._nt, ns._nx) == ((1, 1, 1), ((2, 2, 0), (2, 2, 0), (1, 1, 0))) and ns._pde_desc().eq_weights == (1.0, 1.0, 4.0)
    assert len(ns._term_coefs) == 14 and ns._pde_desc().desc.n_terms == 14
    ch = ns._manual_chain(100)
    assert ch["components"] == 3 and ch["n_bc"] == 2 and len(ch["terms"]) == 4 and ch["x"].shape == (4 * 16 + 25, 2)
    assert [t_[2] for t_ in ch["terms"]] == [0, 1, 0, 1] and float(ch["terms"][1][4][0]) == 0.5
    # trig, coordinates, a single field
    one = P.TermPDESystem(_config(), "w", [[(1.0, ("w_tt",)), (9.81, ("sin(w)",)), (0.1, ("x", "t", "cos(w)"))]], lambda x: x[:, 0])
    assert one._nt == (2,) and one._nx == ((0, 0, 0),) and one._pde_desc().terms[2] == ("x", "t", (0, "cos(u)"))


def test_constructor_refusals_name_the_class():
    ok = dict(fields=("u", "v"), equations=GRAY_SCOTT, initial_condition_fn=_ic2)

    def make(cfg=None, **kw):
        return P.TermPDESystem(cfg or _config(), **dict(ok, **kw))

    for bad in (("u", "v_1"), ("u", "x"), ("u", "t"), ("u", "2v"), ("u", "u"), (), ("a", "b", "c", "d", "e")):
        with pytest.raises(ValueError, match="TermPDESystem: .*field"):
            make(fields=bad)
    with pytest.raises(ValueError, match="TermPDESystem: 5 equations"):
        make(equations=[[(1.0, ("u",))]] * 5)
    with pytest.raises(ValueError, match="TermPDESystem: 33 terms"):
        make(equations=[[(1.0, ("u",))] * 17, [(1.0, ("v",))] * 16])
    with pytest.raises(ValueError, match="TermPDESystem: equation 0, term 0 has 5 factors"):
        make(equations=[[(1.0, ("u",) * 5)]])
    for name in ("w", "u_xy", "u_xxy", "u_yyy", "u_", "sin(w)", "tan(u)", "u_xxxxx"):
        with pytest.raises(ValueError, match=r"TermPDESystem: equation 0, term 0: unknown factor.*mixed derivatives are not available"):
            make(equations=[[(1.0, (name,))]])
    for name in ("u_y", "y", "v_zz"):
        with pytest.raises(ValueError, match="TermPDESystem: .*needs dimension"):
            make(equations=[[(1.0, (name,))]])
    with pytest.raises(NotImplementedError, match="TermPDESystem: the factors of field 'v' need time order 2 together with order 4"):
        make(equations=[[(1.0, ("v_tt",)), (1.0, ("v_xxxx",)), (1.0, ("u",))]])
    with pytest.raises(NotImplementedError, match="TermPDESystem: dimension 4"):
        make(cfg=_with_dimension(4))
    with pytest.raises(TypeError, match="TermPDESystem: initial_condition_fn"):
        make(initial_condition_fn=None)
    with pytest.raises(ValueError, match="TermPDESystem: equation_weights"):
        make(equation_weights=(1.0, -2.0))
    with pytest.raises(ValueError, match="TermPDESystem: equation_weights"):
        make(equation_weights=(1.0,))
    with pytest.raises(ValueError, match="TermPDESystem: initial_condition_fields names 'w'"):
        make(initial_condition_fields=("u", "w"))
    with pytest.raises(ValueError, match="TermPDESystem: dirichlet value"):
        make(cfg=_config(1, {"dirichlet": {"type": "fixed", "value": [0.0, 1.0, 2.0]}}))
    with pytest.raises(NotImplementedError, match="TermPDESystem: dirichlet boundary of type"):
        make(cfg=_config(1, {"dirichlet": {"type": "sine"}}))
    with pytest.raises(NotImplementedError, match="TermPDESystem: boundary conditions"):
        make(cfg=_config(1, {"neumann": {}}))
    with pytest.raises(NotImplementedError, match=r"TermPDESystem: the boundary / initial chain has 16 loss terms \(12 boundary \+ 4 initial\)"):
        P.TermPDESystem(_config(3), ("a", "b", "c", "d"), [[(1.0, ("a",))]], lambda x: x[:, :1].repeat(1, 4))
    with pytest.raises(NotImplementedError, match="TermPDESystem: trainable parameters"):
        make(cfg=_config(trainable_parameters=["Du"]))
    with pytest.raises(ValueError, match="TermPDESystem: coefficient parameter 'missing'"):
        make(equations=[[((1.0, "missing"), ("u",))]])
    with pytest.raises(ValueError, match="TermPDESystem: initial_condition_fn returned"):
        make(initial_condition_fn=lambda x: x[:, 0])._system_points()


def _with_dimension(dim):
    cfg = _config()
    cfg.dimension = dim
    return cfg


class _Stub(torch.nn.Module):
    def __init__(self, din, output_dim):
        super().__init__()
        self.lin = torch.nn.Linear(din, output_dim)
        self.output_dim = output_dim

    def forward(self, inp):
        return self.lin(inp)


def test_trainer_routing_and_refusals():
    """Adam with fixed loss weights, L-BFGS, the uniform and the stratified sampler take the launch list (1-D and 2-D: the
    "multi-dimensional problem" refusal is lifted for the class); everything else is refused with a reason naming the class."""
    from pinnrl_amd.config import AdaptiveWeightsConfig, CausalWeightingConfig, Config, TrainingConfig
    from pinnrl_amd.training import PDETrainer

    def trainer(kind="adam", adaptive=None, causal=False, sampler="uniform", dim=1, out=None):
        cfg = Config.__new__(Config)
        cfg.device = CPU
        cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, optimizer=kind)
        cfg.training.collocation_distribution = sampler
        if adaptive:
            cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy=adaptive, alpha=0.7, eps=1e-6)
        if causal:
            cfg.training.causal_weighting = CausalWeightingConfig(enabled=True, num_bins=8, eps=1.0)
        if dim == 1:
            pc = _config()
            pc.training = cfg.training
            pde = P.TermPDESystem(pc, ("u", "v"), GRAY_SCOTT, _ic2)
        else:
            pc = _config(2, {"dirichlet": {"type": "fixed", "value": [0.0, 0.0, None]}})
            pc.training = cfg.training
            pde = P.TermPDESystem(pc, ("u", "v", "p"), NAVIER_STOKES, lambda x: x[:, :2], initial_condition_fields=("u", "v"))
        return PDETrainer(_Stub(dim + 1, out if out is not None else pde.n_fields), pde, {}, cfg, device=CPU)

    for kind in ("adam", "lbfgs", "adam_lbfgs"):
        for sampler in ("uniform", "stratified"):
            for dim in (1, 2):
                assert trainer(kind, sampler=sampler, dim=dim)._manual_step_unsupported() is None, (kind, sampler, dim)
    whys = {"adaptive": trainer(adaptive="rbw")._manual_step_unsupported(), "causal": trainer(causal=True)._manual_step_unsupported(),
            "sampler": trainer(sampler="residual_based")._manual_step_unsupported(), "model": trainer(out=1)._manual_step_unsupported()}
    tr = trainer()
    tr.process_group = object()
    whys["group"] = tr._manual_step_unsupported()
    tr = trainer()
    tr.rl_agent = object()
    whys["agent"] = tr._manual_step_unsupported()
    tr = trainer()
    tr.pde._trainable_params["Du"] = torch.nn.Parameter(torch.tensor(0.1))
    whys["trainable"] = tr._manual_step_unsupported()
    tr = trainer()
    tr.pde.observation_data = {"x": torch.zeros(1, 1)}
    whys["data"] = tr._manual_step_unsupported()
    for key, word in (("adaptive", "adaptive loss weights"), ("causal", "causal weighting"), ("group", "process group"),
                      ("agent", "RL agent"), ("sampler", "residual-based sampler"), ("trainable", "trainable parameters"),
                      ("data", "data mode"), ("model", "output_dim is 1")):
        assert whys[key] is not None and whys[key].startswith("TermPDESystem") and word in whys[key], (key, whys[key])
    with pytest.raises(NotImplementedError, match="TermPDESystem with adaptive loss weights"):
        trainer(adaptive="rbw").make_graphed_step(64)
    # a model with another output count is refused by the class itself, too
    with pytest.raises(ValueError, match="TermPDESystem: 2 fields .* need a model with output_dim = 2"):
        trainer().pde.compute_loss(_Stub(2, 1), torch.zeros(4, 1), torch.zeros(4, 1))


def test_validate_reports_the_relative_error_over_all_fields():
    exact = lambda x, t: torch.stack([torch.sin(x[:, 0]) * torch.exp(-t[:, 0]), torch.cos(x[:, 0]) + t[:, 0]], 1)  # noqa: E731
    pde = P.TermPDESystem(_config(), ("u", "v"), GRAY_SCOTT, _ic2, exact_solution_fn=exact)

    class Off(torch.nn.Module):
        def forward(self, inp):
            return exact(inp[:, :1], inp[:, 1:]) * 1.01

    torch.manual_seed(0)
    out = pde.validate(Off(), 200)
    assert out["relative_l2_error"] == pytest.approx(0.01, rel=1e-4) and out["max_error"] > 0.0 and set(out) >= {"l2_error", "mean_error"}
    with pytest.raises(ValueError, match=r"expected \(n, 2\)"):
        P.TermPDESystem(_config(), ("u", "v"), GRAY_SCOTT, _ic2, exact_solution_fn=lambda x, t: x).validate(Off(), 10)
