"""`face_conditions=` without a GPU: key resolution (face over axis over default), every refusal of the constructor, a callable
value of the wrong length, term order and count, the signs of the outward normal in the launch-list table, the 32-term cap, the
clash with `config.boundary_conditions`, the unchanged chain descriptions of the config forms, and a zero boundary loss in fp64
for the exact solution of the all-Neumann heat problem."""

import math

import pytest
import torch

import pinnrl_amd  # noqa: F401
from pinnrl_amd import pdes as P
from pinnrl_amd.config import Config, TrainingConfig
from pinnrl_amd.pdes.face_conditions import FaceConditions, FaceTerm
from pinnrl_amd.training import PDETrainer

CPU = torch.device("cpu")
PI = math.pi
HEAT2D = [(1.0, ("u_t",)), ((-1.0, "alpha"), ("u_xx",)), ((-1.0, "alpha"), ("u_yy",))]
HEAT3D = HEAT2D + [((-1.0, "alpha"), ("u_zz",))]
D0 = {"type": "dirichlet", "value": 0.0}
N0 = {"type": "neumann", "value": 0.0}


def _ic(x):
    return torch.prod(torch.cos(PI * x), dim=1)


def _config(dim=2, bcs=None, training=None):
    return P.PDEConfig(name="faces", domain=[(0.0, 1.0)] * dim, time_domain=(0.0, 0.5), parameters={"alpha": 0.1},
                       boundary_conditions=bcs if bcs is not None else {}, initial_condition={}, exact_solution={}, dimension=dim,
                       device=CPU, training=training)


def _nd(fc, dim=2, nb=3, ni=4, **kw):
    return P.TermPDEnD(_config(dim, **kw), HEAT3D if dim == 3 else HEAT2D, _ic, boundary_points_per_axis=nb,
                       initial_points_per_axis=ni, face_conditions=fc)


def _system(fc, dim=2, fields=("u", "v", "p"), ic_fields=("u", "v"), nb=3, ni=4, **kw):
    eqs = [[(1.0, (f"{f}_t",)), (-0.1, (f"{f}_xx",))] for f in fields]
    ic = lambda x: torch.stack([_ic(x)] * len(ic_fields), 1)  # noqa: E731
    return P.TermPDESystem(_config(dim, **kw), fields, eqs, ic, initial_condition_fields=ic_fields, boundary_points_per_axis=nb,
                           initial_points_per_axis=ni, face_conditions=fc)


def test_key_resolution_face_over_axis_over_default():
    robin = {"type": "robin", "alpha": 2.0, "beta": 0.5, "value": 0.2}
    fc = FaceConditions("T", {"default": D0, "y": N0, "y_hi": robin, "x_lo": None}, 2)
    assert fc.terms == [
        FaceTerm(0, 0, 1, 1.0, 0.0, 0.0),    # x_hi: the default; x_lo is an explicit None
        FaceTerm(0, 1, 0, 0.0, -1.0, 0.0),   # y_lo: the axis; outward normal -d/dy
        FaceTerm(0, 1, 1, 2.0, 0.5, 0.2),    # y_hi: the face; outward normal +d/dy
    ]
    # a periodic axis: one paired value term, and one paired derivative term when asked for
    fc = FaceConditions("T", {"default": {"type": "periodic"}, "z": {"type": "periodic", "derivative": True}, "x": D0}, 3)
    assert [(t.axis, t.side, t.alpha, t.beta) for t in fc.terms] == [(0, 0, 1.0, 0.0), (0, 1, 1.0, 0.0), (1, None, 1.0, 0.0),
                                                                    (2, None, 1.0, 0.0), (2, None, 0.0, 1.0)]
    # systems: a spec for every field, or a mapping; a field the mapping leaves out follows the next less specific key
    fc = FaceConditions("T", {"default": {"u": D0, "v": D0, "p": None}, "y_hi": {"u": {"type": "dirichlet", "value": 1.0}},
                              "x_hi": {"p": N0}}, 2, ("u", "v", "p"))
    assert len(fc) == 9
    assert [(t.field, t.axis, t.side) for t in fc.terms] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0),
                                                             (1, 1, 1), (2, 0, 1)]
    assert fc.terms[3].value == 1.0 and fc.terms[7].value == 0.0 and fc.terms[8] == FaceTerm(2, 0, 1, 0.0, 1.0, 0.0)
    # a low-face Neumann / Robin condition carries -d/dx_a
    fc = FaceConditions("T", {"default": {"type": "robin", "alpha": 1.0, "beta": 3.0}}, 2)
    assert [t.beta for t in fc.terms] == [-3.0, 3.0, -3.0, 3.0]


def test_constructor_refusals():
    bad = {
        "dimension 2": {"default": D0, "z": N0},
        "names axis 'z'": {"default": D0, "z_lo": N0},
        "key 'left'": {"default": D0, "left": N0},
        "neither a spec nor None": {"x": D0, "y_lo": D0},          # y_hi resolves to nothing
        "'x_lo'.*periodic pairs the two faces": {"default": D0, "x_lo": {"type": "periodic"}},
        "type 'flux'": {"default": {"type": "flux"}},
        "not \\['gamma'\\]": {"default": {"type": "dirichlet", "gamma": 1.0}},
        "robin needs a finite float 'beta'": {"default": {"type": "robin", "alpha": 1.0}},
        "robin needs a finite float 'alpha'": {"default": {"type": "robin", "alpha": float("inf"), "beta": 1.0}},
        "alpha = beta = 0": {"default": {"type": "robin", "alpha": 0.0, "beta": 0.0}},
        "a finite number or a callable": {"default": {"type": "neumann", "value": "hot"}},
        "'derivative' is True or False": {"default": {"type": "periodic", "derivative": 1}},
        "a spec \\{'type': ...\\} or None": {"default": {"u": D0}},   # a mapping, and TermPDEnD has no field names
        "periodic on one face": {"x": {"type": "periodic"}, "x_hi": D0, "y": D0},
    }
    for match, fc in bad.items():
        with pytest.raises(ValueError, match=match):
            _nd(fc)
    with pytest.raises(TypeError, match="face_conditions is a dict"):
        _nd([D0])
    with pytest.raises(ValueError, match="none of the fields"):
        _system({"default": {"w": D0}})
    with pytest.raises(ValueError, match="face 'y_hi' of field 'p'"):
        _system({"default": {"u": D0, "v": D0}, "x": {"p": None}, "y_lo": {"p": N0}})
    # the two boundary arguments together
    for cls in (_nd, _system):
        with pytest.raises(ValueError, match="both given"):
            cls({"default": D0}, bcs={"dirichlet": {"type": "fixed", "value": 0.0}})
    # without face_conditions the config forms refuse as they always did, word for word
    for cls in (_nd, _system):
        with pytest.raises(NotImplementedError, match="Neumann and Robin faces read derivative streams on the faces: not available"):
            cls(None, bcs={"neumann": {"value": 0.0}})
        with pytest.raises(NotImplementedError, match="boundary conditions \\[\\]"):
            cls(None)
    mixed = P.TermPDEMixed(_config(), [(1.0, ("u_t",)), (-0.1, ("u_xy",))], _ic, face_conditions={"default": N0})
    assert len(mixed._faces) == 4  # TermPDEMixed inherits the keyword


def test_the_term_cap_counts_boundary_and_initial_terms():
    four = ("u", "v", "p", "q")
    per = {"type": "periodic", "derivative": True}
    # 4 fields x 3 axes x (value + derivative) = 24 boundary terms, + 4 initial: 28
    pde = _system({"default": per}, dim=3, fields=four, ic_fields=four, nb=2, ni=2)
    assert len(pde._faces) == 24
    # the largest table of face terms: 4 fields x 6 faces = 24, + 4 initial
    pde = _system({"default": D0}, dim=3, fields=four, ic_fields=four, nb=2, ni=2)
    assert len(pde._faces) == 24 and len(pde._manual_chain(10)["face"]["terms"]) == 28
    # so four fields in three dimensions stay below the cap of 32; the constructors' check itself refuses a larger count
    from pinnrl_amd.pdes.face_conditions import check_term_count
    check_term_count("T", 28, 4)
    with pytest.raises(ValueError, match="33 loss terms \\(29 boundary \\+ 4 initial\\).*at most 32"):
        check_term_count("T", 29, 4)
    # above the old cap of 8 and fine: the issue's cavity, 9 boundary + 2 initial terms
    wall = D0
    cav = _system({"default": {"u": wall, "v": wall, "p": None}, "y_hi": {"u": {"type": "dirichlet", "value": 1.0}}, "x_hi": {"p": N0}})
    ch = cav._manual_chain(10)
    assert ch["n_bc"] == 9 and len(ch["face"]["terms"]) == 11 and ch["terms"] == []
    # and the config form keeps its cap and its message
    with pytest.raises(NotImplementedError, match="one pinn_jet_losses call takes at most 8"):
        _system(None, dim=3, fields=four, ic_fields=four, bcs={"periodic": {}})


def test_callable_values_are_evaluated_once_on_the_face_and_checked():
    calls = []

    def hot(x, t):
        calls.append((x.shape, t.shape))
        return torch.sin(PI * x[:, 1]) * (1 + t[:, 0])

    pde = _nd({"default": N0, "x_lo": {"type": "dirichlet", "value": hot}})
    pts = pde._nd_points()
    assert pde._nd_points() is pts and calls == [((9, 2), (9, 1))]  # nf = 3^2 points of one face, once
    tg = pts["face_targets"]
    assert len(tg) == 4 and tg[1:] == [0.0, 0.0, 0.0]
    xf, tf = pts["x"][:9], pts["t"][:9]
    assert torch.all(xf[:, 0] == 0.0) and torch.equal(tg[0], hot(xf, tf).float())
    bad = _nd({"default": N0, "x_hi": {"type": "dirichlet", "value": lambda x, t: x[:4, 0]}})
    with pytest.raises(ValueError, match="face 'x_hi' returned 4 values for 9 points"):
        bad._nd_points()


def test_the_launch_list_table():
    """2-D, nb = 3 (nf = 9), ni = 4: x_lo Dirichlet, x_hi Robin, y periodic with the derivative."""
    tc = TrainingConfig(learning_rate=1e-3)
    tc.loss_weights = {"pde": 2.0, "boundary": 3.0, "initial": 5.0}
    pde = _nd({"x_lo": D0, "x_hi": {"type": "robin", "alpha": 1.0, "beta": 0.5, "value": 0.2},
               "y": {"type": "periodic", "derivative": True}}, training=tc)
    ch = pde._manual_chain(64)
    pts = pde._nd_points()
    nf, nbc, n = 9, 36, 36 + 16
    assert (ch["nt"], ch["nx"], ch["n_bc"], ch["terms"]) == (0, 0, 4, []) and ch["x"] is pts["x"]
    face = ch["face"]
    # launches (lo, hi, nt, nx, axis, component): the values on all fixed points; d/dx on the x faces through the set (1, 1)
    # (axis 0 has no space-only set), d/dy on the y faces through (0, 1) along axis 1
    assert face["launches"] == [(0, n, 0, 0, 0, 0), (0, 2 * nf, 1, 1, 0, 0), (2 * nf, 4 * nf, 0, 1, 1, 0)]
    t0, t1, t2, t3, t4 = face["terms"]
    assert t0 == {"n": nf, "alpha": 1.0, "beta": 0.0, "target": 0.0, "weight": 3.0, "value": (0, 0, 0)}
    # x_hi: +d/dx, row 2 of the (1, 1) launch [u, u_t, u_x], second face of the launch
    assert t1 == {"n": nf, "alpha": 1.0, "beta": 0.5, "target": 0.2, "weight": 3.0, "value": (0, 0, nf), "deriv": (1, 2, nf)}
    assert t2 == {"n": nf, "alpha": 1.0, "beta": 0.0, "target": 0.0, "weight": 3.0, "value": (0, 0, 2 * nf), "value_pair": (0, 0, 3 * nf)}
    assert t3 == {"n": nf, "alpha": 0.0, "beta": 1.0, "target": 0.0, "weight": 3.0, "deriv": (2, 1, 0), "deriv_pair": (2, 1, nf)}
    assert t4 == {"n": 16, "alpha": 1.0, "beta": 0.0, "target": pts["u0"], "weight": 5.0, "value": (0, 0, nbc)} and t4["target"] is pts["u0"]
    # the outward normal on a low face: -d/dx_a
    lo = _nd({"default": None, "x_lo": {"type": "neumann", "value": 1.0}, "y_lo": {"type": "robin", "alpha": 1.0, "beta": 2.0}})
    f = lo._manual_chain(64)["face"]
    assert [(t.get("alpha"), t["beta"]) for t in f["terms"][:2]] == [(0.0, -1.0), (1.0, -2.0)]
    assert f["terms"][0]["deriv"] == (1, 2, 0) and "value" not in f["terms"][0] and f["terms"][1]["deriv"] == (2, 1, 0)
    # a field without any value term gets no value launch: p with one Neumann face and no initial condition
    cav = _system({"default": {"u": D0, "v": D0, "p": None}, "x_hi": {"p": N0}})
    launches = cav._manual_chain(64)["face"]["launches"]
    assert launches == [(0, n, 0, 0, 0, 0), (0, n, 0, 0, 0, 1), (0, 2 * nf, 1, 1, 0, 2)]


def test_config_forms_keep_their_chain_descriptions():
    """With face_conditions=None the chain of each class is what it was before the keyword existed (literals of that commit)."""
    nf, nbc, nic = 9, 36, 16
    for cls_kw in (dict(), dict(mixed=True)):
        for bcs in ({"dirichlet": {"type": "fixed", "value": 0.25}}, {"periodic": {}}):
            if cls_kw:
                pde = P.TermPDEMixed(_config(bcs=bcs), [(1.0, ("u_t",)), (-0.1, ("u_xy",))], _ic, boundary_points_per_axis=3,
                                     initial_points_per_axis=4)
            else:
                pde = _nd(None, bcs=bcs)
            ch, pts = pde._manual_chain(50), pde._nd_points()
            assert sorted(ch) == ["n_bc", "nt", "nx", "t", "terms", "x"] and (ch["nt"], ch["nx"]) == (0, 0)
            assert ch["x"] is pts["x"] and ch["t"] is pts["t"] and "face_targets" not in pts
            if "dirichlet" in bcs:
                assert ch["n_bc"] == 1 and [tm[:4] + tm[5:] for tm in ch["terms"]] == [(0, nbc, 0, 0, 10.0), (nbc, nbc + nic, 0, 0, 10.0)]
                assert ch["terms"][0][4] is pts["ub"] and torch.all(pts["ub"] == 0.25) and ch["terms"][1][4] is pts["u0"]
            else:
                assert ch["n_bc"] == 2 and ch["terms"][:2] == [(0, nf, 0, nf, None, 10.0), (2 * nf, 3 * nf, 0, nf, None, 10.0)]
                assert ch["terms"][2][:4] + ch["terms"][2][5:] == (nbc, nbc + nic, 0, 0, 10.0) and ch["terms"][2][4] is pts["u0"]
    sysd = _system(None, bcs={"dirichlet": {"type": "fixed", "value": [0.0, 1.0, None]}})
    ch, pts = sysd._manual_chain(50), sysd._system_points()
    assert sorted(ch) == ["components", "n_bc", "nt", "nx", "t", "terms", "x"] and ch["components"] == 3 and ch["n_bc"] == 2
    assert [tm[:4] + tm[5:] for tm in ch["terms"]] == [(0, nbc, 0, 0, 10.0), (0, nbc, 1, 0, 10.0), (nbc, nbc + nic, 0, 0, 10.0),
                                                      (nbc, nbc + nic, 1, 0, 10.0)]
    assert ch["terms"][1][4] is pts["ub"][1] and ch["terms"][3][4].data_ptr() == pts["u0"][1].data_ptr()
    sysp = _system(None, fields=("u", "v"), bcs={"periodic": {}})
    ch = sysp._manual_chain(50)
    assert ch["n_bc"] == 4 and ch["terms"][:4] == [(0, nf, 0, nf, None, 10.0), (2 * nf, 3 * nf, 0, nf, None, 10.0),
                                                   (0, nf, 1, nf, None, 10.0), (2 * nf, 3 * nf, 1, nf, None, 10.0)]


class _Exact(torch.nn.Module):
    """u = exp(-2 alpha pi^2 t) cos(pi x) cos(pi y) in fp64, with `jets` by autograd: the written-out formula behind
    `compute_loss`' boundary terms, on the CPU."""

    output_dim = 1

    def __init__(self, alpha):
        super().__init__()
        self.alpha = alpha

    def u(self, x, t):
        return torch.exp(-2 * self.alpha * PI**2 * t[:, 0]) * torch.cos(PI * x[:, 0]) * torch.cos(PI * x[:, 1])

    def forward(self, inp):
        inp = inp.double()
        return self.u(inp[:, :-1], inp[:, -1:]).reshape(-1, 1)

    def jets(self, x, t, time_order=0, space_order=0, component=0, axis=0):
        x, t = x.double().requires_grad_(True), t.double().requires_grad_(True)
        u = self.u(x, t)
        rows = [u]
        if time_order:
            rows.append(torch.autograd.grad(u.sum(), t, create_graph=True)[0][:, 0])
        if space_order:
            rows.append(torch.autograd.grad(u.sum(), x, create_graph=True)[0][:, axis])
        assert time_order <= 1 and space_order <= 1
        return torch.stack(rows)


def test_all_neumann_faces_vanish_on_the_exact_solution(monkeypatch):
    alpha = 0.1
    pde = _nd({"default": N0}, nb=5, ni=6)
    monkeypatch.setattr(pde, "_residual_loss", lambda model, x, t, n_total=None: torch.zeros((), dtype=torch.float64))
    model = _Exact(alpha)
    out = pde.compute_loss(model, torch.zeros(4, 2), torch.zeros(4, 1))
    # four terms, each the mean of (-+ du/dx_a)^2 over a face where cos(pi x_a)' = -pi sin(pi x_a) = 0 up to sin(pi) in fp64
    assert 0.0 <= float(out["boundary"].detach()) < 1e-28, float(out["boundary"].detach())
    assert float(out["initial"].detach()) < 1e-12  # the initial targets are fp32
    # and the conditions bite: Dirichlet 0 on the same field does not vanish, and is 2 dim means instead of one
    dirichlet = _nd({"default": D0}, nb=5, ni=6)
    monkeypatch.setattr(dirichlet, "_residual_loss", lambda model, x, t, n_total=None: torch.zeros((), dtype=torch.float64))
    b_faces = float(dirichlet.compute_loss(model, torch.zeros(4, 2), torch.zeros(4, 1))["boundary"].detach())
    config_form = _nd(None, nb=5, ni=6, bcs={"dirichlet": {"type": "fixed", "value": 0.0}})
    monkeypatch.setattr(config_form, "_residual_loss", lambda model, x, t, n_total=None: torch.zeros((), dtype=torch.float64))
    b_config = float(config_form.compute_loss(model, torch.zeros(4, 2), torch.zeros(4, 1))["boundary"].detach())
    assert b_config > 1e-2 and b_faces == pytest.approx(4 * b_config, rel=1e-12)


def test_the_trainer_routes_face_conditions_like_the_config_forms():
    def trainer(pde, dim, kind="adam"):
        cfg = Config.__new__(Config)
        cfg.device = CPU
        cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, optimizer=kind)
        pde.config.training = cfg.training
        model = torch.nn.Linear(dim + 1, 1)
        return PDETrainer(model, pde, {}, cfg, device=CPU)

    for kind in ("adam", "lbfgs"):
        assert trainer(_nd({"default": N0}), 2, kind)._manual_step_unsupported() is None
    tr = trainer(_nd({"default": N0}), 2)
    tr.process_group = object()
    assert "process group" in tr._manual_step_unsupported()
