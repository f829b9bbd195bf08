"""CPU tests (no GPU) of the PDE epilogue's cells (tests/epilogue_cells.py):

* `tests/jet_model.py::pde_residual` / `pde_coef_grads`, the executable restatement of `csrc/jet_device.h`, against the
  fp64 reference of every cell at dimensions 1, 2 and 3: the residual on oracle jets, dr/d(jet_s) against autograd of the
  formula, dr/dc against autograd through the reference with live coefficients;
* the conditions every comparison of tests/test_pde_epilogue_gpu.py rests on (no sign flip under mae, both Huber
  branches populated, the clamp mask on and off) for the networks and seeds that file uses;
* routing, from the queries alone: every (cell, lane) takes the kernel family the lane claims, and every `case` of
  `pde_residual` sits on every kernel family that compiles its stream set."""

import pytest
import torch

import epilogue_cells as C
import jet_model as J

DIMS = (1, 2, 3)
MODEL_CELLS = [(k, 1) for k in C.KINDS_1D] + [(k, d) for d in (2, 3) for k in C.KINDS_ND]


def _grad(y, wrt):
    g = torch.autograd.grad(y, wrt, grad_outputs=torch.ones_like(y), create_graph=True, allow_unused=True)[0]
    return torch.zeros_like(y) if g is None else g


def _oracle_jets(spec, params, x, t, nt, nx):
    """[u, u_t .., u_x ..] by chained autograd through the oracle's forward, fp64 (space streams: 1-D only)."""
    import oracle as O

    x, t = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
    u = O.network_forward(spec, params, torch.cat([x, t], 1))
    jets, g = [u], u
    for _ in range(nt):
        g = _grad(g, t)
        jets.append(g)
    g = u
    for _ in range(nx):
        g = _grad(g, x)
        jets.append(g)
    return [j.detach() for j in jets]


def _model_params(kind):
    """The coefficient mapping jet_model reads, as plain floats."""
    k = C.base_kind(kind)
    p = {"L": 1.0} if k == "pendulum" else {}
    for name, c in zip(C.COEF[k][0], C.coef_values(kind)):
        p[name] = [c] if name == "velocity" else c
    return p


@pytest.mark.parametrize("kind,dim", MODEL_CELLS, ids=[C.cell_id(k, d) for k, d in MODEL_CELLS])
def test_jet_model_epilogue_matches_the_reference(kind, dim):
    import oracle as O

    k = C.base_kind(kind)
    spec = O.ArchSpec("feedforward", input_dim=dim + 1, hidden_dim=16, num_layers=2)
    sd = O.init_state_dict(spec, seed=77 + dim)
    x, t = C.points(kind, dim)
    if kind == "cahn_hilliard_clamped":
        sd = C.clamped_state_dict(spec, sd, x, t)
    params = {n: v.double() for n, v in sd.items()}
    x, t = x.double(), t.double()
    live = [torch.tensor(c, dtype=torch.float64, requires_grad=True) for c in C.coef_values(kind)[: len(C.COEF[k][1])]]
    r_ref = C.residual_live(kind, dim, spec, params, live, x, t)
    nt, nx = C.streams(kind, dim)
    assert (nt, nx) == J.pde_streams(k, dim)
    jets = [j.requires_grad_(True) for j in _oracle_jets(spec, params, x, t, nt, nx)]
    x0 = x[:, 0:1]
    p = _model_params(kind)
    r, d = J.pde_residual(k, p, jets, x0, nt, nx, dim)
    scale = max(1.0, float(r_ref.detach().abs().max()))
    err = float((r.detach() - r_ref.detach()).abs().max())
    print(f"{C.cell_id(kind, dim)}: residual max abs err {err:.2e} (scale {scale:.2e})")
    assert err <= 1e-10 * scale
    if kind == "cahn_hilliard_clamped":
        u = jets[0].detach()
        assert int((u.abs() > 10).sum()) >= 5 and int((u.abs() <= 10).sum()) >= 5  # both sides of the mask
    # dr/dj_s: the hand-written cotangents against autograd of the formula
    auto = torch.autograd.grad(r.sum(), jets, allow_unused=True)
    for s, (a, h) in enumerate(zip(auto, d)):
        a = torch.zeros_like(h) if a is None else a
        assert float((a - h.detach()).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max())), f"dr/dj_{s}"
    # dr/dc_k per point: autograd through the reference with live coefficients, identically-zero ones included
    dc = J.pde_coef_grads(k, p, [j.detach() for j in jets], x0, nt, nx, dim)
    want = [torch.zeros(C.N, dtype=torch.float64), torch.zeros(C.N, dtype=torch.float64)]
    for n in range(C.N):
        if live:
            g = torch.autograd.grad(r_ref[n, 0], live, retain_graph=True, allow_unused=True)
            for c, gc in enumerate(g):
                want[c][n] = 0.0 if gc is None else float(gc)
    for c in range(2):
        got = dc[c].flatten()
        if float(want[c].abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, f"dr/dc_{c} must vanish identically"
        else:
            e = float((got - want[c]).abs().max())
            assert e <= 1e-10 * max(1.0, float(want[c].abs().max())), f"dr/dc_{c}: {e:.2e}"


def test_convection_is_refused_beyond_one_dimension():
    """The reference's convection residual raises for dimension > 1; `pinn_pde_streams` refuses it."""
    from pinnrl_amd import engine as E

    with pytest.raises(NotImplementedError):
        E.pde_streams(E.pde_desc("convection", 2, [0.8]))
    assert E.pde_streams(E.pde_desc("convection", 1, [0.8])) == (1, 1)


NETS = sorted({(k, d, C.LANE_NET[lane]) for k, d, lane in C.CASES})


@pytest.mark.parametrize("kind,dim,net", NETS, ids=[f"{C.cell_id(k, d)}-{n}" for k, d, n in NETS])
def test_conditions_hold_on_the_reference(kind, dim, net):
    """`epilogue_cells.reference` asserts them; here for every (cell, network, seed) the GPU file uses."""
    ref = C.reference(kind, dim, net)
    f = C.condition_figures(kind, ref["r"], ref["u"], ref["delta"])
    print(f"{C.cell_id(kind, dim)} {net}: {f}")
    assert len(ref["r"]) == C.N and ref["delta"] > 0
    assert C.f32(ref["delta"]) == ref["delta"]
    for c in ref["sd"].values():
        assert c.dtype == torch.float32
    dc = ref["mse"]["dc"]
    k = C.base_kind(kind)
    if dim == 1 and k != "kdv":
        assert dc[0] != 0.0
    if k == "black_scholes":
        assert dc[1] != 0.0
    else:
        assert dc[1] == 0.0


def test_cells_cover_the_enumerators():
    from pinnrl_amd import _lib

    assert {C.base_kind(k) for k, _ in C.CELLS} == set(_lib.PDE)
    assert len(C.CELLS) == 20 and len(set(C.CELLS)) == 20
    assert all(c == C.f32(c) for k in C.COEF for c in C.coef_values(k))


# ----------------------------------------------------------------------------------------------------------------------
# routing (queries only)
# ----------------------------------------------------------------------------------------------------------------------
def _listed(unit):
    """pinn_build_info() lists the unit as built in a degraded form: the library does not route to it."""
    from pinnrl_amd import _lib

    return unit + ":" in _lib.build_info()  # the library's own test (csrc/pinn_abi.hip: use_u16)


def _expected(lane, kind, dim):
    """`epilogue_cells.claimed`, with the units this build lists as fallen back replaced by what the library falls back to
    (csrc/pinn_abi.hip: a listed 16-point unit leaves its calls to the 32-point kernel; a listed merged unit to the
    four-stream ones)."""
    fam, inv = C.claimed(lane, kind, dim)
    nt, nx = C.streams(kind, dim)
    plain, coef = _listed(f"jet_u16_{nt}_{nx}_0"), _listed(f"jet_u16c_{nt}_{nx}_0")
    if fam == "u16m" and (plain or coef or _listed("jet_u16m_0") or _listed("jet_u16mc_0")):
        fam = "u16"
    if fam == "u16" and plain:
        fam = "wide"
    if inv == "u16" and coef:
        inv = "wide"
    return fam, inv


def test_every_cell_takes_the_family_its_lane_claims():
    from pinnrl_amd import _lib

    print("pinn_build_info():", repr(_lib.build_info()))
    rows = C.table()
    assert [(r[0], r[1]) for r in rows] == [(C.cell_id(k, d), lane) for k, d, lane in C.CASES]  # a cell is never dropped
    print(f"{'cell':28s} {'lane':10s} {'unit':18s} inverse")
    for (kind, dim, lane), (cid, _, unit, inverse) in zip(C.CASES, rows):
        print(f"{cid:28s} {lane:10s} {unit:18s} {inverse}")
        q = C.route(C.descriptor(lane, dim), kind, dim)
        want = _expected(lane, kind, dim)
        assert (C.family(unit), C.family(inverse)) == want, (cid, lane, unit, inverse, want)
        # forward-only and reverse calls of a descriptor are routed together
        assert C.family(q["forward"]) == C.family(q["reverse"]) == ("u16" if want[0] == "u16m" else want[0]), (cid, lane, q)
        if want[0] == "u16":
            nt, nx = C.streams(kind, dim)
            assert unit == f"jet_u16_{nt}_{nx}_0"
    for lane in C.LANES:
        assert {(k, d) for k, d, l in C.CASES if l == lane} == set(C.lane_cells(lane))
    assert set(C.lane_cells("lm")) == set(C.lane_cells("wide64")) == set(C.CELLS)
    assert set(C.lane_cells("u16")) == {(k, d) for k, d in C.CELLS if C.streams(k, d) in C.U16_SETS}


def test_every_branch_runs_on_every_family_that_compiles_its_stream_set():
    """Families: the layer-major head (and the by-value coefficient path on it), the 32-point kernel and its COEF units, the
    16-point units and their COEF units, the merged Burgers units.  A unit this build lists as fallen back is not required
    (its cells are then on the family the query names)."""
    rows = C.table()
    on = {}  # branch -> {family of the residual-mode calls} and {"c" + family of the inverse call}
    for (kind, dim, lane), (_, _, unit, inverse) in zip(C.CASES, rows):
        s = on.setdefault(C.branch(kind, dim), set())
        s.add(C.family(unit))
        s.add("c" + C.family(inverse))
        if lane == "lm":
            s.add("by_value")  # pinn_residual_loss_grad_coef runs on every cell of the layer-major lane
    assert sorted(on) == C.BRANCHES
    for b in C.BRANCHES:
        kind, dim = next((k, d) for k, d in C.CELLS if C.branch(k, d) == b)
        s = C.streams(kind, dim)
        need = {"lm", "clm", "by_value", "wide"}
        if s in C.WIDEC_SETS:
            need.add("cwide")
        if s in C.U16_SETS and not _listed(f"jet_u16_{s[0]}_{s[1]}_0"):
            need.add("u16")
        if s in C.U16C_SETS and not _listed(f"jet_u16c_{s[0]}_{s[1]}_0"):
            need.add("cu16")
        if b == "burgers" and _expected("u16", "burgers", 1)[0] == "u16m":
            need.add("u16m")
        print(f"{b:24s} streams {s}: on {sorted(on[b])}, needs {sorted(need)}")
        assert need <= on[b], (b, sorted(need - on[b]))
    # the clamp mask's m = 0 side cannot run at height 128 (K = 6): it is on the two lanes that compile (1, 4)
    assert {l for k, d, l in C.CASES if k == "cahn_hilliard_clamped"} == {"lm", "wide64"}
