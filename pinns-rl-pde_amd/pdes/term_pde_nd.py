"""`TermPDEnD`: a residual given as data in two or three space dimensions, with derivatives along every space axis.

The jet kernels differentiate along t and along ONE space axis per launch.  A launch whose descriptor carries
`PINN_FLAG_SPACE_AXIS(a)` seeds its space streams from column a of x, so u_y, u_yy (u_z, u_zz) come from one more launch
per axis, and `pinn_term_residual_axes` combines the streams of all launches into

    r = sum_m c_m prod_f phi_{m,f},   phi in TermPDE's factors + {u_y, u_yy, u_z, u_zz, y, z},

with one block of cotangents per launch for the reverse sweeps.  Residual, loss and gradient stay free of autograd, so the
launch list, the captured step, the flat L-BFGS closure and the residual-based sampler take such a PDE as they take
`TermPDE`.  Mixed derivatives (u_xy) and orders above two on the axes y and z are not available here: `TermPDEMixed`
(term_pde_mixed.py) adds them.

Boundary and initial conditions are the class's own: the nine compiled classes keep the reference's behaviour in >= 2-D, where
its boundary points do not fit the model.  Here every face of the box carries a tensor grid of the other coordinates and of
time, and the initial condition a tensor grid of the box at `time_domain[0]`; all of them are fixed and built once.
"""

from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from .. import engine as _E
from .face_conditions import FaceConditions, check_face_arguments, check_term_count
from .pde_base import PDEBase, PDEConfig, _pick_stream_set
from .term_pde import _T_ORDER, _X_ORDER, Coef

_AXIS_ORDER = {"u_y": (1, 1), "u_yy": (1, 2), "u_z": (2, 1), "u_zz": (2, 2)}  # factor -> (axis, order)
_PAIR_AXES = ((0, 1), (0, 2), (1, 2))  # the pairs of axes a mixed factor can name (`engine.MixedTermDesc`)
_COORD_AXIS = {"x": 0, "y": 1, "z": 2}


def box_points(domain, time_domain, dim: int, nb: int, ni: int, dev: torch.device) -> Dict[str, Any]:
    """The fixed boundary and initial points of a box in `dim` space dimensions (1-D: the two ends times the time grid, and the
    line at t0).  x (n, dim), t (n, 1): [face (axis 0, low) | face (axis 0, high) | face (axis 1, low) | ... | initial points];
    every face is the tensor grid of the other coordinates and of time (nb points each: nb^dim per face, the two faces of an
    axis in the same order, so point k of the low face pairs with point k of the high one); the initial points xi are the
    tensor grid of the box (ni per axis) at time_domain[0].  n_face, n_bc = 2 dim n_face, n_ic."""
    t0, t1 = float(time_domain[0]), float(time_domain[1])
    lin = [torch.linspace(domain[d][0], domain[d][1], nb, device=dev) for d in range(dim)]
    tl = torch.linspace(t0, t1, nb, device=dev)
    xs, ts = [], []
    for a in range(dim):
        others = [lin[d] for d in range(dim) if d != a] + [tl]
        mesh = [g.reshape(-1) for g in torch.meshgrid(*others, indexing="ij")]
        for side in (0, 1):
            cols, k = [], 0
            for d in range(dim):
                if d == a:
                    cols.append(torch.full_like(mesh[0], float(domain[a][side])))
                else:
                    cols.append(mesh[k])
                    k += 1
            xs.append(torch.stack(cols, dim=1))
            ts.append(mesh[-1].reshape(-1, 1))
    n_face = nb ** dim
    gi = [torch.linspace(domain[d][0], domain[d][1], ni, device=dev) for d in range(dim)]
    xi = torch.stack([g.reshape(-1) for g in torch.meshgrid(*gi, indexing="ij")], dim=1)
    xs.append(xi)
    ts.append(torch.full((xi.shape[0], 1), t0, device=dev))
    return {"x": torch.cat(xs, 0).float().contiguous(), "t": torch.cat(ts, 0).float().contiguous(), "xi": xi, "n_face": n_face,
            "n_bc": 2 * dim * n_face, "n_ic": xi.shape[0]}


class TermPDEnD(PDEBase):
    """`TermPDEnD(config, terms, initial_condition_fn, exact_solution_fn=None)` for `config.dimension` 2 or 3.

    terms: `[(coef, factors), ...]` as for `TermPDE`; the factor names are TermPDE's plus "u_y", "u_yy", "u_z", "u_zz", "y",
    "z" ("u_x" .. "u_xxxx" and "x" refer to the first axis; the z names need dimension 3).
    initial_condition_fn(x: (n, dim)) -> (n,): the initial value, evaluated once on the fixed initial points.
    exact_solution_fn(x: (n, dim), t: (n, 1)) -> (n,) or (n, 1): enables `validate()`.

    config.boundary_conditions is `{"dirichlet": {"type": "fixed", "value": v}}` (u = v on every face) or `{"periodic": {}}`
    (u on opposite faces paired point by point).  The boundary loss is the mean of l(u - v) over all face points, or the sum
    over the axes of the mean of l(u_low - u_high).

    face_conditions (with an empty config.boundary_conditions) gives every face its own condition instead: Dirichlet, Neumann or
    Robin with a number or a callable as the value, periodic axes with or without the derivative, None for no condition; the
    boundary loss is then the SUM of one mean per face, so {"default": {"type": "dirichlet", "value": v}} is 2 dim times the
    config form's loss (face_conditions.py has the keys and the specs).  An insulated plate, heated through x_lo, cooled by
    convection at x_hi:  face_conditions={"y": {"type": "neumann", "value": 0.0},
                                          "x_lo": {"type": "dirichlet", "value": lambda x, t: torch.sin(torch.pi * x[:, 1])},
                                          "x_hi": {"type": "robin", "alpha": 1.0, "beta": 0.5, "value": 0.2}}

    2-D heat:  TermPDEnD(cfg, [(1.0, ("u_t",)), ((-1.0, "alpha"), ("u_xx",)), ((-1.0, "alpha"), ("u_yy",))],
                         lambda x: torch.sin(torch.pi * x[:, 0]) * torch.sin(torch.pi * x[:, 1]))
    """

    KIND = "term_nd"  # not a `_lib.PDE` kind: the descriptor is an `AxisTermDesc`
    # what a subclass with more factors replaces (TermPDEMixed): the factor names, the (axis, order) of the names beyond
    # TermPDE's, the (pair, order) of the mixed names, and the tail of the unknown-factor message
    _FACTORS = _lib.TERM_FACTOR_ND
    _AXIS_ORDER = _AXIS_ORDER
    _PAIR_ORDER: Dict[str, Tuple[int, int]] = {}
    _FACTOR_NOTE = "mixed derivatives and orders above two along y and z are not available"

    def __init__(self, config: PDEConfig, terms: Sequence[Tuple[Coef, Sequence[str]]],
                 initial_condition_fn: Callable[[torch.Tensor], torch.Tensor],
                 exact_solution_fn: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None,
                 boundary_points_per_axis: int = 16, initial_points_per_axis: int = 32,
                 face_conditions: Optional[Dict[str, Any]] = None, **kwargs):
        dim = int(getattr(config, "dimension", 1))
        if dim not in (2, 3):
            raise NotImplementedError(f"{type(self).__name__}: dimension {dim}: two or three space dimensions (TermPDE runs 1-D problems)")
        if not callable(initial_condition_fn):
            raise TypeError(f"{type(self).__name__}: initial_condition_fn(x: (n, dim)) -> (n,) is required (the reference's 1-D initial "
                            "condition kinds have no n-D form)")
        if int(boundary_points_per_axis) < 2 or int(initial_points_per_axis) < 2:
            raise ValueError(f"{type(self).__name__}: at least 2 boundary and 2 initial points per axis")
        terms = list(terms)
        if len(terms) > _lib.PINN_TERM_MAX_TERMS:
            raise ValueError(f"{type(self).__name__}: {len(terms)} terms; a residual has at most {_lib.PINN_TERM_MAX_TERMS}")
        self._term_coefs: List[Coef] = []
        self._term_factors: List[Tuple[str, ...]] = []
        nt, nx, pair = 0, [0, 0, 0], [0, 0, 0]
        for m, (coef, factors) in enumerate(terms):
            factors = (factors,) if isinstance(factors, str) else tuple(factors)
            if len(factors) > _lib.PINN_TERM_MAX_FACTORS:
                raise ValueError(f"{type(self).__name__}: term {m} has {len(factors)} factors; a term has at most {_lib.PINN_TERM_MAX_FACTORS}")
            for f in factors:
                if f not in self._FACTORS:
                    raise ValueError(f"{type(self).__name__}: term {m}: unknown factor '{f}' (one of {', '.join(self._FACTORS)}; "
                                     f"{self._FACTOR_NOTE})")
                axis = self._AXIS_ORDER[f][0] if f in self._AXIS_ORDER else _COORD_AXIS.get(f, 0)
                if f in self._PAIR_ORDER:
                    axis = _PAIR_AXES[self._PAIR_ORDER[f][0]][1]
                if axis >= dim:
                    raise ValueError(f"{type(self).__name__}: term {m}: factor '{f}' needs dimension {axis + 1}, the problem has {dim}")
                nt = max(nt, _T_ORDER.get(f, 0))
                nx[0] = max(nx[0], _X_ORDER.get(f, 0))
                if f in self._AXIS_ORDER:
                    a, k = self._AXIS_ORDER[f]
                    nx[a] = max(nx[a], k)
                if f in self._PAIR_ORDER:  # u_ab / u_aabb: the pair's launches and the same order on both of its axes
                    j, k = self._PAIR_ORDER[f]
                    pair[j] = max(pair[j], k)
                    for a in _PAIR_AXES[j]:
                        nx[a] = max(nx[a], k)
            if isinstance(coef, (tuple, list)):
                if len(coef) != 2 or not isinstance(coef[1], str):
                    raise ValueError(f"{type(self).__name__}: term {m}: a coefficient is a number or (scale, 'parameter name')")
                coef = (float(coef[0]), coef[1])
            else:
                coef = float(coef)
            self._term_coefs.append(coef)
            self._term_factors.append(factors)
        try:
            self._nt, nx[0] = _pick_stream_set(nt, nx[0])
        except NotImplementedError:
            raise NotImplementedError(
                f"{type(self).__name__}: the factors need time order {nt} together with order {nx[0]} along x, and no compiled stream set "
                "holds both (time order 2 goes with space order 0 or 2)") from None
        self._nx = tuple(nx)
        self._pair = tuple(pair)
        bcs = dict(getattr(config, "boundary_conditions", None) or {})
        self._faces: Optional[FaceConditions] = None
        if face_conditions is not None:
            check_face_arguments(type(self).__name__, face_conditions, config)
            self._faces = FaceConditions(type(self).__name__, face_conditions, dim)
            check_term_count(type(self).__name__, len(self._faces), 1)
            self._bc = ("faces", 0.0)
        elif list(bcs) == ["dirichlet"]:
            p = bcs["dirichlet"] or {}
            if p.get("type", "fixed") != "fixed":
                raise NotImplementedError(f"{type(self).__name__}: dirichlet boundary of type '{p.get('type')}': a fixed value on all faces only")
            self._bc = ("dirichlet", float(p.get("value", 0.0)))
        elif list(bcs) == ["periodic"]:
            self._bc = ("periodic", 0.0)
        else:
            raise NotImplementedError(
                f"{type(self).__name__}: boundary conditions {sorted(bcs)}: exactly one of {{'dirichlet': {{'type': 'fixed', 'value': v}}}} on "
                "all faces or {'periodic': {}} (Neumann and Robin faces read derivative streams on the faces: not available)")
        if list(getattr(config, "trainable_parameters", []) or []):
            raise NotImplementedError(f"{type(self).__name__}: trainable parameters (inverse problems) are not covered: the coefficients of a "
                                      "term residual are read by value")
        super().__init__(config)
        if self._training_mode() != "forward" or self.observation_data:
            raise NotImplementedError(f"{type(self).__name__}: data modes and observation data are not covered (forward problems only)")
        for coef in self._term_coefs:
            if isinstance(coef, tuple) and self.get_parameter(coef[1]) is None:
                raise ValueError(f"{type(self).__name__}: coefficient parameter '{coef[1]}' is not in config.parameters")
        self._initial_condition_fn = initial_condition_fn
        self._exact_solution_fn = exact_solution_fn
        self._nb, self._ni = int(boundary_points_per_axis), int(initial_points_per_axis)
        self._coef_values: Optional[torch.Tensor] = None
        self._coef_device: Optional[torch.device] = None
        self._descs: Dict[Any, Any] = {}
        self._points: Optional[Tuple[torch.device, Dict[str, Any]]] = None

    # ---------------------------------------------------------------- coefficients and descriptors
    def _coefficients(self):
        return tuple(c[0] * float(self.get_parameter(c[1], required=True)) if isinstance(c, tuple) else c for c in self._term_coefs)

    def _has_trainable_coefficients(self) -> bool:
        return False

    @property
    def coef_values(self) -> torch.Tensor:
        """The c_m as float32 on the PDE's device, one per term, built once: what the kernel reads at launch time."""
        dev = torch.device(self.device)  # the REQUESTED device is remembered beside the tensor (see TermPDE.coef_values)
        if self._coef_values is None or self._coef_device != dev:
            self._coef_values = torch.tensor([float(c) for c in self._coefficients()], dtype=torch.float32, device=dev).reshape(-1)
            self._coef_device = dev
            self._descs = {}
        return self._coef_values

    def _term_desc(self, loss: str, delta: float) -> "_E.AxisTermDesc":
        cv = self.coef_values
        key = (loss, float(delta))
        if key not in self._descs:
            self._descs[key] = _E.AxisTermDesc(self._term_factors, cv, self.dimension, self._nt, self._nx, loss, delta)
        return self._descs[key]

    def _pde_desc(self):
        return self._term_desc(self._loss_function_name(), self._huber_delta())

    def _pde_desc_l1(self):
        return self._term_desc("mae", 1.0)

    def exact_solution(self, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        if self._exact_solution_fn is None:
            raise NotImplementedError(f"{type(self).__name__}: no exact_solution_fn was given")
        return self._exact_solution_fn(x, t).reshape(-1, 1)

    # ---------------------------------------------------------------- fixed evaluation points
    def _nd_points(self) -> Dict[str, Any]:
        """The fixed boundary and initial points, built once per device.
        x (n, dim), t (n, 1): [face (axis 0, low) | face (axis 0, high) | face (axis 1, low) | ... | initial points];
        every face is the tensor grid of the other coordinates and of time (nb points each: nb^dim per face, the two faces
        of an axis in the same order, so point k of the low face pairs with point k of the high one); the initial points are
        the tensor grid of the box (ni per axis) at time_domain[0].  n_face, n_bc = 2 dim n_face, n_ic; u0: the initial
        targets, (n_ic,)."""
        dev = torch.device(self.device)
        if self._points is not None and self._points[0] == dev:
            return self._points[1]
        pts = box_points(self.domain, self.time_domain, self.dimension, self._nb, self._ni, dev)
        xi = pts.pop("xi")
        with torch.no_grad():
            u0 = self._initial_condition_fn(xi).reshape(-1).float().contiguous()
        if u0.shape[0] != xi.shape[0]:
            raise ValueError(f"{type(self).__name__}: initial_condition_fn returned {u0.shape[0]} values for {xi.shape[0]} points")
        pts["u0"] = u0.to(dev)
        if self._bc[0] == "dirichlet":
            pts["ub"] = torch.full((pts["n_bc"],), self._bc[1], dtype=torch.float32, device=dev)
        if self._faces is not None:
            pts["face_targets"] = self._faces.targets(type(self).__name__, pts)
        self._points = (dev, pts)
        return pts

    # ---------------------------------------------------------------- losses
    def compute_loss(self, model, x: torch.Tensor, t: torch.Tensor, n_total: Optional[int] = None,
                     aux_scale: float = 1.0) -> Dict[str, torch.Tensor]:
        """The residual loss of `PDEBase._residual_loss` (the chain behind `engine.residual_loss_grad`), the boundary and
        the initial loss on the fixed points of `_nd_points` from ONE forward of the model, and `_compose_losses`' tail."""
        dev = self.device
        residual_loss = self._residual_loss(model, x, t, n_total)
        P = self._nd_points()
        u = model(torch.cat([P["x"], P["t"]], dim=1)).reshape(-1)
        nbc, nf = P["n_bc"], P["n_face"]
        if self._faces is not None:
            boundary_loss = self._faces.boundary_loss(self, model, P, P["face_targets"], u.reshape(-1, 1))
        elif self._bc[0] == "dirichlet":
            boundary_loss = self._apply_loss_fn(u[:nbc] - P["ub"])
        else:
            boundary_loss = torch.zeros((), device=dev)
            for a in range(self.dimension):
                lo = 2 * a * nf
                boundary_loss = boundary_loss + self._apply_loss_fn(u[lo : lo + nf] - u[lo + nf : lo + 2 * nf])
        initial_loss = self._apply_loss_fn(u[nbc:] - P["u0"])
        zero = torch.zeros((), device=dev)
        return self._compose_losses(residual_loss, boundary_loss, initial_loss, zero, zero, aux_scale)

    def _manual_chain(self, n_batch: int) -> Dict[str, Any]:
        """`compute_loss`' boundary / initial part as data for the launch list (see PDEBase._manual_chain): the value stream
        on the fixed points; one target term over all faces (dirichlet) or one paired term per axis (periodic), then the
        initial term.  With face_conditions: no "terms"; "face" holds the jet launches and the `pinn_face_losses` table
        (`FaceConditions.chain`), the boundary terms first, then the initial term."""
        P = self._nd_points()
        lw = self._loss_weights()
        bw, iw = (lw.get("boundary", 10.0), lw.get("initial", 10.0)) if lw else (10.0, 10.0)
        nbc, nf = P["n_bc"], P["n_face"]
        if self._faces is not None:
            return {"x": P["x"], "t": P["t"], "nt": 0, "nx": 0, "terms": [], "n_bc": len(self._faces),
                    "face": self._faces.chain(P, P["face_targets"], float(bw), [(0, P["u0"], float(iw))])}
        if self._bc[0] == "dirichlet":
            terms = [(0, nbc, 0, 0, P["ub"], float(bw))]
        else:
            terms = [(2 * a * nf, 2 * a * nf + nf, 0, nf, None, float(bw)) for a in range(self.dimension)]
        n_bc_terms = len(terms)
        terms.append((nbc, nbc + P["n_ic"], 0, 0, P["u0"], float(iw)))
        return {"x": P["x"], "t": P["t"], "nt": 0, "nx": 0, "terms": terms, "n_bc": n_bc_terms}
