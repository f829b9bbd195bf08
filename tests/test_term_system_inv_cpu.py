"""CPU tests (no GPU) of learnable parameters and observation data in coupled term systems: `pinn_term_residual_system_inv`,
`engine.InvSystemTermDesc`, `TermPDESystem(..., learn=..., observations=...)` and `TermPDESystemMixed` with them.

(a) the fp64 model of tests/term_system_inv_model.py: its programs are what the kernel test says they are; `param_grads` equals
    the central differences of its own <rbar, r> in fp64 with respect to every parameter; with no learnable entry it is the
    sibling model value for value; the seeds of the kernel test keep the kinks of the loss clear (at most 1 % of the points
    unsafe) and every G and H sum well conditioned (the float32 evaluation in numpy alone stays within half of their 1e-6);
(b) header, `_lib.EXPORTS` and the library agree, still ABI 2, the descriptor's size and offsets, the Makefile rule;
(c) every host-side rejection the entry point adds, with made-up addresses and no device;
(d) `engine.InvSystemTermDesc`: bytes, validation, `launches()` / `blocks()` equal the parent's, `with_loss`;
(e) the PDE classes: the rules of both keywords, descriptor class and bytes unchanged without `learn`, `learned`,
    `learned_values`, `get_parameter`, `trainable_parameters_iter`, the chain with data terms;
(f) the trainer: the launch list under Adam, the L-BFGS reason.
"""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pinnrl_amd  # noqa: F401
import pinnrl_amd.pdes as P
import term_system_inv_model as M
import term_system_nl_model as NM
from pinnrl_amd import _lib
from pinnrl_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# (a) the model
# ---------------------------------------------------------------------------------------------------------------------
def test_programs_are_what_the_kernel_test_says():
    assert sorted(M.PROGRAMS) == ["caps8", "euler1d", "exp1"] and M.SIZES == (1, 255, 256, 257, 64 * 256 + 3)
    dim, nt, nx, pair, n_eq, terms, coef, K, nl, pv, cp, npar = M.PROGRAMS["exp1"]
    assert (dim, len(nt), n_eq) == (1, 1, 1) and [r[0] for r in nl] == ["exp"] and any(q >= 0 for q in cp) and npar[0][0] >= 0
    assert npar[0][1] >= 0 and nl[0][2] != 0.0  # shift and scale learnable, the shift's scale not zero
    dim, nt, nx, pair, n_eq, terms, coef, K, nl, pv, cp, npar = M.PROGRAMS["euler1d"]
    assert [r[0] for r in nl] == ["recip", "pow"] and npar[0][0] >= 0 and npar[1][2] >= 0 and any(q >= 0 for q in cp)
    dim, nt, nx, pair, n_eq, terms, coef, K, nl, pv, cp, npar = M.PROGRAMS["caps8"]
    assert (dim, len(nt), n_eq, len(terms), len(pv)) == (3, 4, 4, 32, 8)
    assert NM.mask_of(terms, [r[:2] for r in nl]) == [0, 1, 2] and npar[3][0] >= 0  # a learnable entry on a masked-out function
    assert cp.count(0) == 3 and npar[2][1] == 0  # one parameter shared by three terms and a nonlinear scale
    assert nl[1][1] == "nl0" and npar[0][0] >= 0 and npar[1][0] >= 0 and npar[0][0] != npar[1][0]  # nl1(nl0(.)), both shifts
    used = {q for q in cp if q >= 0} | {q for r in npar for q in r if q >= 0}
    assert used == set(range(8))
    a = M.inputs("caps8", 255)
    assert np.all(np.isnan(a[13][3]))  # the numbers of the function outside the mask are NaN: never read
    m = M.evaluate(*a[:10], fn=a[11], nonlinear=a[12], nl_params=a[13], param_values=a[14], coef_param=a[15], nl_param=a[16],
                   eq_weights=M.EQ_WEIGHTS["caps8"])
    assert np.all(np.isfinite(m["r"])) and np.all(np.isfinite(m["param_grads"])) and m["param_grads"][3] == 0.0
    # every argument of a restricted function stays in the sibling's domain
    for name in sorted(M.PROGRAMS):
        for N in M.SIZES:
            a = M.inputs(name, N)
            m = M.evaluate(*a[:10], fn=a[11], nonlinear=a[12], nl_params=a[13], param_values=a[14], coef_param=a[15], nl_param=a[16])
            for k, arg in m["nl_args"].items():
                if a[12][k][0] in NM.DOMAIN_OPS:
                    assert 1.5 <= float(arg.min()) and float(arg.max()) <= 4.5, (name, N, k)


@pytest.mark.parametrize("name", sorted(M.PROGRAMS))
def test_param_grads_are_the_central_differences_of_the_models_pairing(name):
    dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, pv, cp, npar = M.inputs(name, 7, seed=5)
    m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, pv, cp, npar, residual_cotangent=rbar, exact=True)
    h = 1e-6
    for p in range(len(pv)):
        L = []
        for s in (1.0, -1.0):
            q = pv.astype(np.float64).copy()
            q[p] += s * h
            L.append(M.pairing(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, q, cp, npar, rbar))
        fd = (L[0] - L[1]) / (2 * h)
        assert abs(fd - m["param_grads"][p]) <= 1e-7 * max(m["param_abs"][p], 1e-12), (p, fd, m["param_grads"][p])
        inside = any(q == p for q in cp) or any(r[j] == p and k in m["mask"] for k, r in enumerate(npar) for j in range(3))
        assert (m["param_abs"][p] > 0) == inside
    # and each H on its own: d <rbar, r> / d (effective entry) by central differences of the sibling model
    en = m["eff_nl"]
    for k in m["mask"]:
        for j in range(3 if nl[k][0] == "pow" else 2):
            L = []
            for s in (1.0, -1.0):
                e2 = en.copy()
                e2[k, j] += s * h
                r = NM.evaluate(dim, nt, nx, pair, n_eq, terms, m["eff_coef"], jets, x, t, fn, nl, e2)["r"]
                L.append(float((rbar.astype(np.float64) * r).sum()))
            assert abs((L[0] - L[1]) / (2 * h) - m["H"][k, j]) <= 1e-7 * max(m["H_abs"][k, j], 1e-12), (k, j)


def test_no_learnable_entry_is_the_sibling_model_value_for_value():
    for name in sorted(NM.PROGRAMS):
        dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params = NM.inputs(name, 255)
        for loss, delta in M.LOSSES:
            s = NM.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, NM.EQ_WEIGHTS[name], loss, delta, 0.1)
            for pv in (None, np.asarray([2.0, 3.0], dtype=np.float32)):  # parameters that nothing names change nothing
                m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, pv, None, None,
                               NM.EQ_WEIGHTS[name], loss, delta, 0.1)
                for k in ("r", "r_bound", "rbar", "rbar_bound", "coef_sums", "coef_abs", "eq_loss", "unsafe", "count"):
                    assert np.array_equal(m[k], s[k], equal_nan=True), k
                for k in ("cot", "cot_bound", "touched"):
                    assert all((a is None and b is None) or np.array_equal(a, b, equal_nan=True) for a, b in zip(m[k], s[k])), k
                assert not m["param_grads"].any() and m["param_grads"].shape == (0 if pv is None else 2,)


def test_the_seeds_keep_the_kinks_clear_and_the_sums_well_conditioned():
    for name in sorted(M.PROGRAMS):
        for N in M.SIZES:
            dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, rbar, fn, nl, params, pv, cp, npar = M.inputs(name, N)
            for loss, delta in M.LOSSES:
                if loss == "mse":
                    continue
                m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, pv, cp, npar, M.EQ_WEIGHTS[name],
                               loss, delta, 1.0 / N)
                assert m["unsafe"].any(0).sum() <= 0.01 * N, (name, N, loss)
            m = M.evaluate(dim, nt, nx, pair, n_eq, terms, coef, jets, x, t, fn, nl, params, pv, cp, npar, residual_cotangent=rbar)
            G, H = M.sums_fp32(dim, nt, nx, pair, terms, coef, jets, x, t, fn, nl, params, pv, cp, npar, rbar)
            assert np.all(np.abs(G - m["coef_sums"]) <= 0.5 * M.SUM_TOL * m["coef_abs"]), (name, N)
            assert np.all(np.abs(H - m["H"]) <= 0.5 * M.SUM_TOL * m["H_abs"]), (name, N)
            assert not H[[k for k in range(len(nl)) if k not in m["mask"]]].any()  # a function outside the mask contributes 0


# ---------------------------------------------------------------------------------------------------------------------
# (b) header, binding, library
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pinn_jet.h")).read()
    assert re.search(r"\bint pinn_term_residual_system_inv\s*\(", hdr) and re.search(r"typedef struct PinnTermPdeSystemInv\b", hdr)
    assert "pinn_term_residual_system_inv" in _lib.EXPORTS and hasattr(_lib.load(), "pinn_term_residual_system_inv")
    assert _lib.load().pinn_abi_version() == 2 == _lib.PINN_ABI_VERSION and re.search(r"#define PINN_ABI_VERSION 2\b", hdr)
    assert re.search(r"#define PINN_SYSTEM_MAX_PARAMS 8\b", hdr) and _lib.PINN_SYSTEM_MAX_PARAMS == 8
    assert re.search(r"#define PINN_SYSTEM_INV_SCRATCH_DOUBLES \(64 \* \(4 \+ 32 \+ 12\)\)", hdr)
    assert _lib.PINN_SYSTEM_INV_SCRATCH_DOUBLES == 64 * 48
    S, F = _lib.PinnTermPdeSystemInv, _lib.PinnTermPdeSystemNl
    assert ctypes.sizeof(S) == ctypes.sizeof(F) + 4 * (1 + 32 + 12)
    for name, _ in F._fields_:  # the fields of the sibling, in its order, at its offsets
        assert getattr(S, name).offset == getattr(F, name).offset and getattr(S, name).size == getattr(F, name).size, name
    assert [n for n, _ in S._fields_][: len(F._fields_)] == [n for n, _ in F._fields_]
    assert S.n_params.offset == ctypes.sizeof(F) and S.coef_param.offset == ctypes.sizeof(F) + 4
    assert S.nl_param.offset == ctypes.sizeof(F) + 4 + 4 * 32
    members = re.search(r"typedef struct PinnTermPdeSystemInv \{(.*?)\} PinnTermPdeSystemInv;", hdr, re.S).group(1)
    members = re.sub(r"/\*.*?\*/", "", members, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[[^;]*)?;", members) == [n for n, _ in S._fields_]
    proto = re.search(r"int pinn_term_residual_system_inv\((.*?)\);", hdr, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"\s+", " ", proto).split(",")]
    sib = re.search(r"int pinn_term_residual_system_nl\((.*?)\);", hdr, re.S).group(1)
    want = [a.split()[-1].lstrip("*") for a in re.sub(r"\s+", " ", sib).split(",")]
    want.insert(want.index("nl_params") + 1, "param_values")
    want.insert(want.index("coef_grads") + 1, "param_grads")
    assert names == want and len(_lib.load().pinn_term_residual_system_inv.argtypes) == len(names)
    mk = open(os.path.join(ROOT, "pinns-rl-pde_amd", "csrc", "Makefile")).read()
    assert mk.count("build/term_system_inv_kernels.o") >= 4 and "term_system_inv_kernels: uses scratch" in mk
    assert "term_system_inv_kernels: spills vector registers" in mk
    assert os.path.exists(os.path.join(ROOT, "pinns-rl-pde_amd", "csrc", "term_system_inv_kernels.hip"))


# ---------------------------------------------------------------------------------------------------------------------
# (c) host-side validation
# ---------------------------------------------------------------------------------------------------------------------
def _desc(P_=2, cp=(0, -1), npar=((1, -1, -1), (-1, -1, -1)), nl=((4, (1, 0)), (2, (0, 31)))):
    """A raw descriptor: 2 fields in 2-D, two terms (the second names nl1, whose source is nl0: both are evaluated); nl0 is a POW."""
    d = _lib.PinnTermPdeSystemInv()
    d.dimension, d.n_fields, d.n_equations, d.n_terms, d.n_functions, d.n_nonlinear = 2, 2, 2, 2, 0, len(nl)
    for c in range(2):
        d.time_order[c] = 1
        d.space_order[c][0], d.space_order[c][1] = 2, 2
    d.eq_weight[0] = d.eq_weight[1] = 1.0
    d.loss, d.huber_delta = 0, 1.0
    for m, (e, factors) in enumerate(((0, ((0, 1),)), (1, ((1, 3), (1, 31))))):
        d.equation_of[m] = e
        d.terms[m].n_factors = len(factors)
        for f, (field, code) in enumerate(factors):
            d.terms[m].factor[f] = field * 32 + code
    for k, (op, (field, code)) in enumerate(nl):
        d.nl_op[k], d.nl_source[k] = op, field * 32 + code
    d.n_params = P_
    for m in range(32):
        d.coef_param[m] = cp[m] if m < len(cp) else -1
    for k in range(4):
        for j in range(3):
            d.nl_param[k][j] = npar[k][j] if k < len(npar) else -1
    return d


def _call(d, pv=0x1000, pg=None, scratch=None, cot=None, N=8, nlp=0x1000):
    lib = _lib.load()
    jets = (ctypes.c_void_p * 12)(0x1000, 0x2000, None, 0x3000, 0x4000, None, None, None, None, None, None, None)
    return lib.pinn_term_residual_system_inv(ctypes.byref(d), 0x1000, jets, 0x1000, 0x1000, None, nlp, pv, N, 1.0, None, None, None, None,
                                             cot, None, pg, scratch, None)


def test_validation_is_answered_on_the_host():
    """Every rejection comes back before any HIP call: the addresses are made up and there is no device."""
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "pinn_jet.h")).read()
    BAD = int(re.search(r"PINN_ERR_BAD_DESC\s*=\s*(-?\d+)", hdr).group(1))
    MIS = int(re.search(r"PINN_ERR_MISALIGNED\s*=\s*(-?\d+)", hdr).group(1))
    err = lambda: lib.pinn_last_error().decode()  # noqa: E731
    assert lib.pinn_term_residual_system_inv(None, 0x1000, None, None, None, None, None, None, 8, 1.0, None, None, None, None, None, None,
                                             None, None, None) == BAD and "null descriptor" in err()
    assert _call(_desc(), N=0) == 0  # the descriptor is good: N == 0 is a no-op
    for n in (-1, 9):
        assert _call(_desc(P_=n)) == BAD and "n_params" in err() and "[0, 8]" in err()
    for q in (-2, 2, 8):
        assert _call(_desc(cp=(-1, q))) == BAD and "term 1: coef_param" in err() and "[-1, 2)" in err(), q
    assert _call(_desc(P_=0, npar=((-1, -1, -1),) * 2)) == BAD and "term 0: coef_param 0 outside [-1, 0)" in err()
    for j, word in enumerate(("shift", "scale", "exponent")):
        for q in (-2, 2):
            row = [-1, -1, -1]
            row[j] = q
            assert _call(_desc(npar=(tuple(row), (-1, -1, -1)))) == BAD and "nonlinear function 0" in err() and word in err(), (j, q)
    assert _call(_desc(npar=((1, -1, 0), (-1, -1, -1))), N=0) == 0  # a learnable exponent on the POW
    assert _call(_desc(npar=((1, -1, -1), (-1, -1, 0)))) == BAD and "nonlinear function 1: a learnable exponent needs PINN_NL_POW" in err()
    # entries beyond n_terms / n_nonlinear are not read
    d = _desc()
    d.coef_param[2] = 99
    d.nl_param[2][0] = 99
    assert _call(d, N=0) == 0
    # null param_values with any index >= 0; fine when every index is -1
    assert _call(_desc(), pv=None) == BAD and "term 0 has a learnable coefficient but param_values is null" in err()
    assert _call(_desc(cp=(-1, -1)), pv=None) == BAD and "nonlinear function 0 has a learnable entry but param_values is null" in err()
    assert _call(_desc(cp=(-1, -1), npar=((-1, -1, -1),) * 2), pv=None, N=0) == 0
    # param_grads without scratch; misaligned scratch
    assert _call(_desc(), pg=0x1000) == BAD and "param_grads without scratch" in err()
    assert _call(_desc(), pg=0x1000, scratch=0x1004) == MIS and "8-byte" in err()
    # every check of the sibling still answers, under this entry point's name
    assert _call(_desc(), nlp=None) == BAD and "nonlinear function 0 is evaluated but nl_params is null" in err()
    assert _call(_desc(nl=((10, (1, 0)), (2, (0, 31))))) == BAD and "nonlinear function 0: unknown operation" in err()
    d = _desc()
    d.n_terms = 33
    assert _call(d) == BAD and "n_terms" in err() and err().startswith("pinn_term_residual_system_inv:")
    tab = (ctypes.c_void_p * 12)(0x1000, None, None, 0x3000, 0x4000, None, None, None, None, None, None, None)
    assert _call(_desc(), cot=tab) == BAD and "(field 0, axis 1)" in err()


# ---------------------------------------------------------------------------------------------------------------------
# (d) the engine object
# ---------------------------------------------------------------------------------------------------------------------
def _td(name, loss="mse", delta=1.0, cls=E.InvSystemTermDesc):
    dim, nt, nx, pair, n_eq, terms, coef, K, nl, pv, cp, npar = M.PROGRAMS[name]
    factors, eq_of = M.engine_terms(terms)
    rows = M.engine_nonlinear([r[:2] for r in nl], [r[2:] for r in nl])
    fns = [lambda x, t: x[:, 0]] * K
    if cls is E.NlSystemTermDesc:
        return cls(factors, eq_of, torch.tensor(coef), dim, len(nt), n_eq, nt, nx, pair, fns, rows, M.EQ_WEIGHTS[name], loss, delta)
    return cls(factors, eq_of, torch.tensor(coef), dim, len(nt), n_eq, nt, nx, pair, fns, rows, M.EQ_WEIGHTS[name], loss, delta,
               param_values=torch.tensor(pv, dtype=torch.float32), coef_param=cp, nl_param=npar)


def test_inv_system_term_desc():
    td = _td("euler1d", "huber", 0.5)
    d = td.desc
    assert isinstance(td, E.NlSystemTermDesc) and isinstance(d, _lib.PinnTermPdeSystemInv) and d.n_params == 3
    assert list(d.coef_param) == [-1] * 8 + [0, 0] + [-1] * 22
    assert [list(r) for r in d.nl_param] == [[1, -1, -1], [-1, -1, 2], [-1, -1, -1], [-1, -1, -1]]
    # the sibling's bytes, then the maps
    tn = _td("euler1d", "huber", 0.5, cls=E.NlSystemTermDesc)
    n = ctypes.sizeof(_lib.PinnTermPdeSystemNl)
    assert bytes(d)[:n] == bytes(tn.desc) and len(bytes(d)) == n + 4 * 45
    tail = np.frombuffer(bytes(d)[n:], dtype=np.int32)
    assert tail[0] == 3 and list(tail[1:33]) == list(d.coef_param) and list(tail[33:39]) == [1, -1, -1, -1, -1, 2]
    for name in sorted(M.PROGRAMS):  # parameters add no network launch
        t1, t0 = _td(name), _td(name, cls=E.NlSystemTermDesc)
        assert t1.launches() == t0.launches() and t1.blocks() == t0.blocks() and E.pde_streams(t1) == E.pde_streams(t0), name
    td2 = td.with_loss("mae")
    assert type(td2) is E.InvSystemTermDesc and td2.param_values is td.param_values and td2.coef_param == td.coef_param
    assert td2.nl_param == td.nl_param and td2.nl_values is td.nl_values and td2.coef_values is td.coef_values
    assert td2.desc.loss == _lib.LOSS["mae"] and bytes(td2.desc)[n:] == bytes(d)[n:]
    c8 = _td("caps8")
    assert c8.desc.n_params == 8 and list(c8.desc.coef_param).count(0) == 3 and [list(r) for r in c8.desc.nl_param][3] == [3, -1, -1]
    # without parameters: the sibling's program, every index -1
    t0 = E.InvSystemTermDesc(td.terms, td.equation_of, td.coef_values, 1, 3, 3, td.nt, td.nx, td.pair, (), td.nonlinear,
                             M.EQ_WEIGHTS["euler1d"])
    assert t0.desc.n_params == 0 and set(t0.desc.coef_param) == {-1} and t0.param_values is None
    assert bytes(t0.desc)[:n] == bytes(_td("euler1d", cls=E.NlSystemTermDesc).desc)
    # validation
    ok = dict(terms=[((0, "u_t"),), ("nl0", (0, "u_xx"))], equation_of=[0, 0], coef_values=torch.zeros(2), dimension=1, n_fields=1,
              n_equations=1, nt=(1,), nx=((2, 0, 0),), nonlinear=[("exp", (0, "u"), 0.0, 1.0, 1.0)], param_values=torch.ones(2),
              coef_param=[0, -1], nl_param=[(1, -1, -1)])
    E.InvSystemTermDesc(**ok)
    bad = lambda **kw: E.InvSystemTermDesc(**dict(ok, **kw))  # noqa: E731
    with pytest.raises(ValueError, match="at most 8 learnable parameters"):
        bad(param_values=torch.ones(9))
    with pytest.raises(ValueError, match=r"param_values: a contiguous float32 \(P,\) tensor"):
        bad(param_values=torch.ones(2, dtype=torch.float64))
    for cp in ([0], [0, 2], [0, -2]):
        with pytest.raises(ValueError, match="coef_param: one entry per term"):
            bad(coef_param=cp)
    for npar in ([], [(2, -1, -1)], [(0, -1)]):
        with pytest.raises(ValueError, match="nl_param: one .* row per nonlinear function"):
            bad(nl_param=npar)
    with pytest.raises(ValueError, match="a learnable exponent needs the operation 'pow'"):
        bad(nl_param=[(-1, -1, 0)])
    # the front end refuses before it looks for a device
    td = E.InvSystemTermDesc(**ok)
    call = lambda pv, pg=None: E.term_residual_system_inv(td, [torch.zeros(4, 5)], None, td.nl_values, pv, torch.zeros(5, 1),  # noqa: E731
                                                          torch.zeros(5), param_grads=pg)
    with pytest.raises(ValueError, match="param_values is None but the descriptor has 2 parameters"):
        call(None)
    with pytest.raises(ValueError, match=r"param_values must be a contiguous float32 \(2,\) tensor"):
        call(torch.ones(3))
    with pytest.raises(ValueError, match="param_grads must hold 2 contiguous float32 values"):
        call(td.param_values, torch.zeros(1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        call(td.param_values)
    with pytest.raises(ValueError, match="only an `InvSystemTermDesc` has learnable parameters"):
        E._term_residual_sys(_td("euler1d", cls=E.NlSystemTermDesc), [torch.zeros(3, 5)], torch.zeros(5, 1), torch.zeros(5),
                             param_grads=torch.zeros(3))


# ---------------------------------------------------------------------------------------------------------------------
# (e) the PDE classes
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(dim=1, bcs=None, **params):
    return P.PDEConfig(name="inv", domain=[(0.0, 1.0)] * dim, time_domain=(0.0, 1.0), parameters=dict(params),
                       boundary_conditions={"periodic": {}} if bcs is None else bcs, initial_condition={}, exact_solution={},
                       dimension=dim, device=CPU)


MONOD = [[(1.0, ("u_t",)), ((-1.0, "D"), ("u_xx",)), ((1.0, "R"), ("u", "m"))]]
MONOD_NL = {"m": ("recip", "u", {"shift": "K"}), "q": ("pow", "u", {"shift": 2.0, "exponent": (0.5, "E")})}
_ic = lambda x: x[:, :1]  # noqa: E731


def _monod(learn, cls=P.TermPDESystem, dim=1, **kw):
    return cls(_cfg(dim, D=0.1, R=2.0, K=0.5, E=3.0), ("u",), MONOD, _ic, nonlinear=MONOD_NL, learn=learn, **kw)


def test_learn_builds_the_maps_and_the_parameter_tensor():
    pde = _monod({"D": 0.05, "K": None, "R": 1.5})
    assert isinstance(pde.learned, torch.nn.Parameter) and pde.learned.shape == (3,) and pde.learned.dtype == torch.float32
    assert pde.learned.tolist() == [pytest.approx(0.05), 0.5, 1.5]  # the order of `learn`; None starts at the config's value
    assert pde.learned_values() == {"D": pytest.approx(0.05), "K": 0.5, "R": 1.5}
    assert pde.get_parameter("D") == pytest.approx(0.05) and pde.get_parameter("E") == 3.0
    assert list(pde.trainable_parameters_iter()) == [pde.learned] and list(pde.trainable_parameters_iter())[0] is pde.learned
    assert not len(pde._trainable_params) and not pde._has_trainable_coefficients() and pde._training_mode() == "forward"
    td = pde._pde_desc()
    assert type(td) is E.InvSystemTermDesc and td.param_values is pde.learned and td.desc.n_params == 3
    assert td.coef_param == (-1, 0, 2) and td.nl_param == ((1, -1, -1), (-1, -1, -1))
    # a learnable entry stores its SCALE; the others their value
    assert pde.coef_values.tolist() == [1.0, -1.0, 1.0] and pde.nl_values.tolist() == [[1.0, 1.0, 1.0], [2.0, 1.0, 1.5]]
    assert pde._pde_desc_l1().param_values is pde.learned and pde._pde_desc_l1().desc.loss == _lib.LOSS["mae"]
    with torch.no_grad():
        pde.learned[0] = 0.25
    assert pde.learned_values()["D"] == 0.25 and pde.get_parameter("D") == 0.25
    # a learnable exponent on pow, with a scale
    pe = P.TermPDESystem(_cfg(1, D=0.1, R=2.0, K=0.5, E=3.0), ("u",), [MONOD[0] + [(1.0, ("q",))]], _ic, nonlinear=MONOD_NL, learn={"E": 2.0})
    assert pe._pde_desc().nl_param == ((-1, -1, -1), (-1, -1, 0)) and pe.nl_values.tolist()[1] == [2.0, 1.0, 0.5]
    # the mixed class takes the keyword and keeps its pair orders
    pm = P.TermPDESystemMixed(_cfg(2, nu=0.1), ("u", "v"), [[(1.0, ("u_t",)), ((-1.0, "nu"), ("v_xy",))], [(1.0, ("v_t",))]], lambda x: x,
                              learn={"nu": None})
    tm = pm._pde_desc()
    assert type(tm) is E.InvSystemTermDesc and tm.pair == pm._pair == ((0, 0, 0), (2, 0, 0)) and tm.coef_param == (-1, 0, -1)


def test_without_learn_the_descriptors_are_what_they_were():
    lin = [[(1.0, ("u_t",)), ((-1.0, "D"), ("u_xx",))]]
    for kw in ({}, {"learn": None}, {"learn": {}}):
        p1 = P.TermPDESystem(_cfg(1, D=0.1), ("u",), lin, _ic, **kw)
        assert type(p1._pde_desc()) is E.SystemTermDesc and p1.learned is None and p1.learned_values() == {}
        assert list(p1.trainable_parameters_iter()) == [] and p1.coef_values.tolist() == [1.0, pytest.approx(-0.1)]
        assert type(P.TermPDESystemMixed(_cfg(2, D=0.1), ("u",), lin, _ic, **kw)._pde_desc()) is E.MixedSystemTermDesc
        assert type(P.TermPDESystem(_cfg(1, D=0.1), ("u",), lin, _ic, functions={"f": lambda x, t: x[:, 0]}, **kw)._pde_desc()) \
            is E.FnSystemTermDesc
        p2 = _monod(kw.get("learn"))
        assert type(p2._pde_desc()) is E.NlSystemTermDesc
        ref = P.TermPDESystem(_cfg(1, D=0.1, R=2.0, K=0.5, E=3.0), ("u",), MONOD, _ic, nonlinear=MONOD_NL)
        assert bytes(p2._pde_desc().desc) == bytes(ref._pde_desc().desc)
        assert torch.equal(p2.coef_values, ref.coef_values) and torch.equal(p2.nl_values, ref.nl_values)
        assert p2.nl_values.tolist() == [[0.5, 1.0, 1.0], [2.0, 1.0, 1.5]]
    # with learn the sibling's bytes are the prefix: the program is the same
    n = ctypes.sizeof(_lib.PinnTermPdeSystemNl)
    assert bytes(_monod({"D": None})._pde_desc().desc)[:n] == bytes(_monod(None)._pde_desc().desc)


def test_learn_refusals():
    with pytest.raises(ValueError, match="learn names 'Z', which is not in config.parameters"):
        _monod({"Z": 1.0})
    with pytest.raises(ValueError, match="learn names 'E', which no term coefficient and no nonlinear"):
        P.TermPDESystem(_cfg(1, D=0.1, R=2.0, K=0.5, E=3.0), ("u",), MONOD, _ic, nonlinear={"m": MONOD_NL["m"]}, learn={"E": 1.0})
    with pytest.raises(ValueError, match="learn names 9 parameters; a system learns at most 8"):
        P.TermPDESystem(_cfg(1, **{f"p{k}": 1.0 for k in range(9)}), ("u",), [[((1.0, f"p{k}"), ("u",)) for k in range(9)]], _ic,
                        learn={f"p{k}": None for k in range(9)})
    with pytest.raises(ValueError, match="nonlinear 'm': the exponent 'E' is learnable, which needs the operation 'pow'"):
        P.TermPDESystem(_cfg(1, D=0.1, R=2.0, K=0.5, E=3.0), ("u",), MONOD, _ic, nonlinear={"m": ("recip", "u", {"exponent": "E"})},
                        learn={"E": 1.0})
    for guess in (float("nan"), float("inf"), "big"):
        with pytest.raises(ValueError, match="a finite initial guess"):
            _monod({"D": guess})
    # what stays refused, exactly as before
    cfg = _cfg(1, D=0.1, R=2.0, K=0.5, E=3.0)
    cfg.trainable_parameters = ["D"]
    with pytest.raises(NotImplementedError, match="trainable parameters"):
        P.TermPDESystem(cfg, ("u",), MONOD, _ic, nonlinear=MONOD_NL, learn={"D": None})
    cfg = _cfg(1, D=0.1, R=2.0, K=0.5, E=3.0)
    cfg.training = {"mode": "inverse"}
    with pytest.raises(NotImplementedError, match="data modes and observation data are not covered"):
        P.TermPDESystem(cfg, ("u",), MONOD, _ic, nonlinear=MONOD_NL, learn={"D": None})


def _obs(n=5, dim=1, k=1, **kw):
    g = torch.Generator().manual_seed(3)
    return dict({"x": torch.rand(n, dim, generator=g), "t": torch.rand(n, 1, generator=g), "u": torch.rand(n, k, generator=g)}, **kw)


WALLS = {"dirichlet": {"type": "fixed", "value": [0.0, 0.0, None]}}  # no boundary term for the pressure
NS = [[(1.0, ("u_t",)), ((1.0, "lam"), ("u", "u_x")), (1.0, ("p_x",)), ((-1.0, "nu"), ("u_xx",))],
      [(1.0, ("v_t",)), ((1.0, "lam"), ("u", "v_x")), (1.0, ("p_y",)), ((-1.0, "nu"), ("v_xx",))],
      [(1.0, ("u_x",)), (1.0, ("v_y",))]]


def test_observations_rules_and_chain():
    mk = lambda obs, bcs=WALLS, **kw: P.TermPDESystem(_cfg(2, bcs=bcs, lam=1.0, nu=0.01), ("u", "v", "p"), NS, lambda x: x,  # noqa: E731
                                                      observations=obs, initial_condition_fields=("u", "v"), **kw)
    assert mk(None)._obs is None
    pde = mk(_obs(5, 2, 2, fields=("u", "v")), learn={"lam": 0.5, "nu": None})
    assert pde._obs["fields"] == (0, 1) and pde._obs["u"].shape == (2, 5) and pde._obs["u"].is_contiguous() and pde._obs["n"] == 5
    assert mk(_obs(5, 2, 3))._obs["fields"] == (0, 1, 2)  # all fields by default
    assert mk(_obs(5, 2, 1, fields="p"))._obs["fields"] == (2,)
    assert pde._training_mode() == "forward" and not pde.observation_data
    for bad, word in ((_obs(5, 1, 2, fields=("u", "v")), r"observations\['x'\] has shape \(5, 1\)"),
                      (dict(_obs(5, 2, 2, fields=("u", "v")), t=torch.zeros(5)), r"observations\['t'\] has shape \(5,\)"),
                      (_obs(5, 2, 3, fields=("u", "v")), r"observations\['u'\] has shape \(5, 3\), expected \(5, 2\)"),
                      (_obs(5, 2, 1, fields=("w",)), "observations names the field 'w'"),
                      (_obs(5, 2, 2, fields=("u", "u")), "none twice"),
                      ({"x": torch.zeros(5, 2)}, "observations is a mapping with"),
                      (dict(_obs(5, 2, 2, fields=("u", "v")), extra=1), "observations is a mapping with")):
        with pytest.raises(ValueError, match=word):
            mk(bad)
    nan = _obs(5, 2, 2, fields=("u", "v"))
    nan["u"][3, 1] = float("nan")
    with pytest.raises(ValueError, match="observations hold NaN or inf"):
        mk(nan)
    cfg = _cfg(2, bcs=WALLS, lam=1.0, nu=0.01)
    cfg.observation_data = {"path": "/nonexistent"}
    with pytest.raises((NotImplementedError, FileNotFoundError)):
        P.TermPDESystem(cfg, ("u", "v", "p"), NS, lambda x: x, observations=_obs(5, 2, 3))
    # the plain chain: the data terms behind the initial ones, their field the stream, on the appended points
    ch = pde._manual_chain(64)
    Pn = pde._system_points()
    n0 = Pn["x"].shape[0]
    assert ch["x"].shape == (n0 + 5, 2) and ch["t"].shape == (n0 + 5, 1) and torch.equal(ch["x"][n0:], pde._obs["x"])
    assert ch["n_data"] == 2 and len(ch["terms"]) == ch["n_bc"] + 2 + 2 and ch["n_bc"] == 2
    for k, term in enumerate(ch["terms"][-2:]):
        assert term[:4] == (n0, n0 + 5, k, 0) and torch.equal(term[4], pde._obs["u"][k]) and term[5] == 1.0
    assert "n_data" not in mk(None)._manual_chain(64) and mk(None)._manual_chain(64)["x"].shape[0] == n0
    # the term count includes the data terms: 6 periodic + 2 initial + 3 data > 8
    with pytest.raises(NotImplementedError, match=r"11 loss terms \(6 boundary \+ 2 initial \+ 3 data\)"):
        mk(_obs(5, 2, 3), bcs={"periodic": {}})
    mk(None, bcs={"periodic": {}})
    # the face chain: the value launch of an observed field is extended, a field without one gets its own; no initial fields at all
    none = {"default": {"u": None, "v": None, "p": None}}
    pf = P.TermPDESystemMixed(_cfg(2, bcs={}, lam=1.0, nu=0.01), ("u", "v", "p"), NS, None, face_conditions=none,
                              initial_condition_fields=(), observations=_obs(5, 2, 2, fields=("u", "v")), learn={"lam": 0.5, "nu": None})
    cf = pf._manual_chain(64)
    nf0 = pf._system_points()["x"].shape[0]
    assert cf["n_data"] == 2 and cf["n_bc"] == 0 and cf["face"]["launches"] == [(nf0, nf0 + 5, 0, 0, 0, 0), (nf0, nf0 + 5, 0, 0, 0, 1)]
    assert [tm["value"] for tm in cf["face"]["terms"]] == [(0, 0, 0), (1, 0, 0)] and all(tm["n"] == 5 for tm in cf["face"]["terms"])
    pg = P.TermPDESystemMixed(_cfg(2, bcs={}, lam=1.0, nu=0.01), ("u", "v", "p"), NS, lambda x: x[:, :1], face_conditions=none,
                              initial_condition_fields=("u",), observations=_obs(5, 2, 2, fields=("u", "v")))
    cg = pg._manual_chain(64)
    assert cg["face"]["launches"] == [(0, nf0 + 5, 0, 0, 0, 0), (nf0, nf0 + 5, 0, 0, 0, 1)]
    assert [tm["value"] for tm in cg["face"]["terms"]] == [(0, 0, pg._system_points()["n_bc"]), (0, 0, nf0), (1, 0, 0)]
    with pytest.raises(TypeError, match="initial_condition_fn"):
        P.TermPDESystem(_cfg(2, lam=1.0, nu=0.01), ("u", "v", "p"), NS, None)


# ---------------------------------------------------------------------------------------------------------------------
# (f) the trainer
# ---------------------------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    def __init__(self, din, output_dim):
        super().__init__()
        self.lin = torch.nn.Linear(din, output_dim)
        self.output_dim = output_dim

    def forward(self, inp):
        return self.lin(inp)


def test_trainer_routing_and_the_lbfgs_reason():
    from pinnrl_amd.config import Config, TrainingConfig
    from pinnrl_amd.training import PDETrainer

    def trainer(kind="adam", sampler="uniform", learn=True, obs=True):
        cfg = Config.__new__(Config)
        cfg.device = CPU
        cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, optimizer=kind)
        cfg.training.collocation_distribution = sampler
        pc = _cfg(2, bcs=WALLS, lam=1.0, nu=0.01)
        pc.training = cfg.training
        pde = P.TermPDESystem(pc, ("u", "v", "p"), NS, lambda x: x, initial_condition_fields=("u", "v"),
                              learn={"lam": 0.5, "nu": None} if learn else None,
                              observations=_obs(5, 2, 2, fields=("u", "v")) if obs else None)
        return PDETrainer(_Stub(3, 3), pde, {}, cfg, device=CPU)

    for sampler in ("uniform", "stratified"):
        tr = trainer(sampler=sampler)
        assert tr._manual_step_unsupported() is None, sampler
        held = [p for g in tr.optimizer.param_groups for p in g["params"]]
        assert any(p is tr.pde.learned for p in held)  # the optimiser holds the parameter tensor
    for kind in ("lbfgs", "adam_lbfgs"):
        why = trainer(kind)._manual_step_unsupported()
        assert why is not None and "learn" in why and "[theta || parameters]" in why, why
        assert trainer(kind, learn=False)._manual_step_unsupported() is None  # observations alone keep the flat L-BFGS
    assert trainer(learn=False, obs=False)._manual_step_unsupported() is None
