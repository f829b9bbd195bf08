"""`TermPDESystem`: a coupled system of PDEs given as data — several unknowns, several equations.

The fields are the outputs of ONE network with `output_dim = C`.  Output k of such a network is exactly the one-output network
whose output layer is row k of the output weight and entry k of the output bias, so the jets of field k come from a component
launch (`engine.jets_forward(..., component=k)`): the layer-major engine with the two output-layer entries of its weight table
(and of its gradient table) pointing at row k.  `pinn_term_residual_system` combines the streams of all fields into

    r_e = sum_{m in equation e} c_m prod_f phi_{m,f},   phi a stream of ANY field, a coordinate, sin / cos of a field,

and hands every (field, axis) block its cotangents for one component reverse sweep each.  Residuals, loss and gradient stay
free of autograd, so the launch list, the captured step and the flat L-BFGS closure take such a system as they take
`TermPDEnD`.  A component launch recomputes the trunk: a C-field system costs about C single-field chains.  Mixed derivatives
(`<field>_xy`) are not available here: `TermPDESystemMixed` (term_pde_system_mixed.py) has them.
"""

from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from .. import engine as _E
from .face_conditions import FaceConditions, check_face_arguments, check_term_count
from .pde_base import PDEBase, PDEConfig, _jets_of, _pick_stream_set
from .term_pde import Coef
from .term_pde_nd import box_points

_SUFFIX = {  # factor suffix -> (the one-field factor name, time order, (axis, space order))
    "": ("u", 0, (0, 0)), "t": ("u_t", 1, (0, 0)), "tt": ("u_tt", 2, (0, 0)),
    "x": ("u_x", 0, (0, 1)), "xx": ("u_xx", 0, (0, 2)), "xxx": ("u_xxx", 0, (0, 3)), "xxxx": ("u_xxxx", 0, (0, 4)),
    "y": ("u_y", 0, (1, 1)), "yy": ("u_yy", 0, (1, 2)), "z": ("u_z", 0, (2, 1)), "zz": ("u_zz", 0, (2, 2)),
}
_COORDS = {"x": 0, "y": 1, "z": 2, "t": -1}
PINN_MAX_POINT_TERMS = 8  # the loss terms one pinn_jet_losses call takes


class TermPDESystem(PDEBase):
    """`TermPDESystem(config, fields, equations, initial_condition_fn, exact_solution_fn=None, equation_weights=None,
    initial_condition_fields=None)` for `config.dimension` 1, 2 or 3.  Mixed derivatives: `TermPDESystemMixed`.

    fields: 1 to 4 names, each an identifier without "_" and none of x, y, z, t; field k is output k of the model, and
        `config.output_dim` is set to their number.
    equations: 1 to 4 term lists `[(coef, factors), ...]` in `TermPDE`'s form (coef a number or `(scale, "parameter name")`), at
        most 32 terms of at most 4 factors over all equations.  Factor names: "<field>", "<field>_t", "<field>_tt",
        "<field>_x" .. "<field>_xxxx", "<field>_y", "<field>_yy", "<field>_z", "<field>_zz", "sin(<field>)", "cos(<field>)", "x",
        "y", "z", "t".  Per field the smallest compiled stream set that holds its factors is launched.
    functions: {name: g} with at most 4 entries: known functions g(x: (n, dim), t: (n, 1)) -> (n,) (the convention of the value
        callables of `face_conditions`) that the terms may name as factors — a source f(x, t), a coefficient kappa(x, y), a
        velocity field, a body force.  A name is an identifier without "_", none of x, y, z, t, sin, cos and no field name; the
        factor "<name>" is the function's value at the point (factor code 27 + k, k the position in the mapping).  A function
        is a factor like a coordinate: it takes part in the products and nothing is differentiated through it — the residual
        has no derivative with respect to x and t through a function, as it has none through a coordinate factor or through the
        network: `compute_residual` detaches the points, they are constants of the residual's graph, and `x.requires_grad`
        yields no gradient through the residual, with functions as without.  Every function is evaluated once per residual call under
        `torch.no_grad()`, also one that no term names.  Under a captured training step a function must be pure device torch ops
        without a host read (no `.item()`, no Python branch on a tensor): torch's own capture error is the refusal.  A function
        may close over a device tensor, and rewriting that tensor in place changes the eager step and the replay.  With
        functions the descriptor is an `engine.FnSystemTermDesc` (`pinn_term_residual_system_fn`); without, it is what it was.
        Forced heat in 1-D, u_t - u_xx = f:
            TermPDESystem(cfg, ("u",), [[(1.0, ("u_t",)), (-1.0, ("u_xx",)), (-1.0, ("f",))]], ic,
                          functions={"f": lambda x, t: torch.exp(-t[:, 0]) * torch.sin(math.pi * x[:, 0]) * (math.pi**2 - 1)})
    nonlinear: {name: (op, source) | (op, source, {"shift": a, "scale": b, "exponent": p})} with at most 4 entries: nonlinear
        functions of the unknowns that the terms may name as factors, "<name>" = g(shift + scale * source) at the point.  op is one
        of exp, log, recip (1 / arg), sqrt, pow (arg ** exponent), tanh, sinh, cosh, sin, cos.  The source is a stream factor name
        of a field ("T", "u_x", in `TermPDESystemMixed` also "v_xy") or the name of an EARLIER entry, so functions nest; the order
        of the mapping is the order of evaluation.  No coordinate, no known function and no sin(<field>) / cos(<field>) is a
        source.  A source's stream counts towards the stream orders of its field exactly as a term factor does.  shift, scale
        and exponent (defaults 0, 1, 1) are a number, a parameter name of config.parameters or (number, "parameter name"); they
        are held in `nl_values`, a (K, 3) float32 device tensor built once beside `coef_values` and read at launch time, so
        rewriting it in place changes the eager step and a captured one.  They are trainable only through `learn` (below).  Names follow the rule for
        functions: an identifier without "_", none of x, y, z, t, sin, cos, no field, no function and no other nonlinear name.
        The gradient flows through g' to the source.  An argument outside the domain of g (log of a negative number, 1 / 0) is
        not checked: NaN or inf spreads into the loss.  ONLY THE VALUE of g is a factor: a space or time derivative of g(u) has
        to be written out by the chain rule by hand, as with sin(<field>).  (kappa(u) u_x)_x = kappa'(u) u_x^2 + kappa(u) u_xx
        needs kappa and kappa' as two declarations; with kappa = exp(u) both are the same one.  With nonlinear the descriptor
        is an `engine.NlSystemTermDesc` (`pinn_term_residual_system_nl`); without, it is what it was.  Bratu-type in 1-D,
        u_t - u_xx - lam e^u, and Monod kinetics u / (K + u):
            TermPDESystem(cfg, ("u",), [[(1.0, ("u_t",)), (-1.0, ("u_xx",)), ((-1.0, "lam"), ("eu",))]], ic,
                          nonlinear={"eu": ("exp", "u")})
            nonlinear={"m": ("recip", "u", {"shift": "K"})}  with the term (1.0, ("u", "m"))
    learn: {name: initial guess | None} with at most 8 names of config.parameters (None: start at the config's value): an inverse
        problem.  A learnable name may stand wherever a parameter name may: a term coefficient (scale, "name"), or shift / scale /
        exponent of `nonlinear` as "name" or (scale, "name") — the exponent under "pow" only.  A name that nothing uses, a name
        missing from config.parameters and more than 8 names are refused.  `pde.learned` is ONE (P,) float32 nn.Parameter on the
        device, in the order of `learn`: the buffer the kernel reads at launch time (for a learnable entry `coef_values` /
        `nl_values` hold the scale, the effective number is scale * parameter).  `trainable_parameters_iter()` yields it, so
        `PDETrainer`'s optimiser holds it; `learned_values()` returns {name: float}, and `get_parameter(name)` of a learnable name
        its current value.  Under autograd `compute_loss(...)["total"].backward()` fills `pde.learned.grad` from the same chain
        and kernel (`engine.ResidualLossParamFunction`); the launch list (Adam, fixed loss weights, eager and captured) steps it
        with one more Adam call, unclipped.  With `learn` the descriptor is an `engine.InvSystemTermDesc`
        (`pinn_term_residual_system_inv`); without, it is what it was.  config.trainable_parameters stays refused.
            TermPDESystem(cfg, ("u",), [[(1.0, ("u_t",)), ((-1.0, "D"), ("u_xx",)), ((1.0, "R"), ("u", "m"))]], ic,
                          nonlinear={"m": ("recip", "u", {"shift": "K"})}, learn={"D": 0.08, "R": None, "K": 2.5})
    observations: {"x": (n, dim), "t": (n, 1), "u": (n, k), "fields": names} — data on k of the fields ("fields" defaults to all;
        fields not named stay hidden, e.g. the pressure).  `compute_loss` returns "data" = sum over the observed fields of
        mean l(u_c(obs) - target_c), which enters "total" with loss_weights["data"] (default 1).  On the launch list the points
        are appended to the fixed points of the boundary / initial chain, one loss term per observed field, and count towards its
        term limit (8, or 32 with face_conditions).  training.mode stays "forward"; config.observation_data and the data modes
        stay refused.  Shapes, unknown field names and NaN / inf are refused here.  `initial_condition_fields=()` (then
        initial_condition_fn may be None) is a problem known from data alone.
    equation_weights: omega_e >= 0 (default 1): the residual loss is sum_e omega_e mean l(r_e).
    initial_condition_fn(x: (n, dim)) -> (n, len(initial_condition_fields)); initial_condition_fields defaults to all fields.
    exact_solution_fn(x, t) -> (n, C): enables `validate()`.

    config.boundary_conditions is `{"periodic": {}}` (every field, opposite faces paired point by point) or
    `{"dirichlet": {"type": "fixed", "value": v}}` with v a number or a list of C entries; an entry None means no boundary
    term for that field (the pressure of incompressible flow).  Boundary and initial losses are sums over the fields.  The
    fixed points are `TermPDEnD`'s: every face a tensor grid of the other coordinates and of time (in 1-D the two ends times
    the time grid), the initial points a tensor grid of the box at `time_domain[0]`.

    face_conditions (with an empty config.boundary_conditions) gives every face of every field its own condition instead
    (face_conditions.py: Dirichlet, Neumann, Robin, periodic, None; a spec for all fields or a mapping {field: spec | None} per
    key); every (face, field) with a condition is one loss term of the boundary sum, and the boundary and initial terms
    together number at most 32.  A lid-driven cavity, with wall = {"type": "dirichlet", "value": 0.0}:
        face_conditions={"default": {"u": wall, "v": wall, "p": None}, "y_hi": {"u": {"type": "dirichlet", "value": 1.0}}}

    Gray-Scott in 1-D:
        TermPDESystem(cfg, ("u", "v"),
                      [[(1.0, ("u_t",)), ((-1.0, "Du"), ("u_xx",)), (1.0, ("u", "v", "v")), ((-1.0, "F"), ()), ((1.0, "F"), ("u",))],
                       [(1.0, ("v_t",)), ((-1.0, "Dv"), ("v_xx",)), (-1.0, ("u", "v", "v")), ((1.0, "Fk"), ("v",))]],
                      lambda x: torch.stack([1 - 0.5 * torch.exp(-50 * x[:, 0] ** 2), 0.25 * torch.exp(-50 * x[:, 0] ** 2)], 1))
    """

    KIND = "term_system"  # not a `_lib.PDE` kind: the descriptor is a `SystemTermDesc`
    # the unknown-factor message: the names a field takes, and what is not available (a subclass with more names has its own)
    _FACTOR_NAMES = "<field>, <field>_t, _tt, _x .. _xxxx, _y, _yy, _z, _zz, sin(<field>), cos(<field>)"
    _FACTOR_NOTE = "mixed derivatives are not available in systems"

    def __init__(self, config: PDEConfig, fields: Sequence[str], equations: Sequence[Sequence[Tuple[Coef, Sequence[str]]]],
                 initial_condition_fn: Callable[[torch.Tensor], torch.Tensor],
                 exact_solution_fn: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None,
                 equation_weights: Optional[Sequence[float]] = None, initial_condition_fields: Optional[Sequence[str]] = None,
                 boundary_points_per_axis: int = 16, initial_points_per_axis: int = 32,
                 face_conditions: Optional[Dict[str, Any]] = None,
                 functions: Optional[Dict[str, Callable[[torch.Tensor, torch.Tensor], torch.Tensor]]] = None,
                 nonlinear: Optional[Dict[str, Sequence[Any]]] = None, learn: Optional[Dict[str, Optional[float]]] = None,
                 observations: Optional[Dict[str, Any]] = None, **kwargs):
        who = type(self).__name__
        dim = int(getattr(config, "dimension", 1))
        if dim not in (1, 2, 3):
            raise NotImplementedError(f"{who}: dimension {dim}: one to three space dimensions")
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        if not 1 <= len(fields) <= _lib.PINN_SYSTEM_MAX_FIELDS:
            raise ValueError(f"{who}: {len(fields)} fields; a system has 1 to {_lib.PINN_SYSTEM_MAX_FIELDS}")
        for name in fields:
            if not isinstance(name, str) or not name.isidentifier() or "_" in name or name in _COORDS:
                raise ValueError(f"{who}: field name {name!r}: an identifier without '_' that is none of x, y, z, t")
        if len(set(fields)) != len(fields):
            raise ValueError(f"{who}: field names {fields} repeat")
        equations = [list(eq) for eq in equations]
        if not 1 <= len(equations) <= _lib.PINN_SYSTEM_MAX_EQUATIONS:
            raise ValueError(f"{who}: {len(equations)} equations; a system has 1 to {_lib.PINN_SYSTEM_MAX_EQUATIONS}")
        n_terms = sum(len(eq) for eq in equations)
        if n_terms > _lib.PINN_SYSTEM_MAX_TERMS:
            raise ValueError(f"{who}: {n_terms} terms over all equations; a system has at most {_lib.PINN_SYSTEM_MAX_TERMS}")
        no_initial = initial_condition_fields is not None and len(tuple(initial_condition_fields)) == 0
        if not callable(initial_condition_fn) and not (no_initial and initial_condition_fn is None):
            raise TypeError(f"{who}: initial_condition_fn(x: (n, dim)) -> (n, number of initial fields) is required")
        if int(boundary_points_per_axis) < 2 or int(initial_points_per_axis) < 2:
            raise ValueError(f"{who}: at least 2 boundary and 2 initial points per axis")
        C = len(fields)
        index = {name: c for c, name in enumerate(fields)}
        self.fields = fields
        functions = dict(functions or {})
        if len(functions) > _lib.PINN_SYSTEM_MAX_FUNCTIONS:
            raise ValueError(f"{who}: {len(functions)} functions; a system names at most {_lib.PINN_SYSTEM_MAX_FUNCTIONS}")
        for name, g in functions.items():
            if (not isinstance(name, str) or not name.isidentifier() or "_" in name or name in _COORDS or name in index
                    or name in ("sin", "cos")):
                raise ValueError(f"{who}: function name {name!r}: an identifier without '_' that is none of x, y, z, t, sin, cos and "
                                 f"no field name ({', '.join(fields)})")
            if not callable(g):
                raise TypeError(f"{who}: function '{name}' is not callable: g(x: (n, dim), t: (n, 1)) -> (n,)")
        self._functions = tuple(functions.items())  # (name, callable); function k is factor code 27 + k
        fn_index = {name: k for k, name in enumerate(functions)}
        self._term_coefs: List[Coef] = []
        self._term_factors: List[Tuple[object, ...]] = []
        self._equation_of: List[int] = []
        nt, nx = [0] * C, [[0, 0, 0] for _ in range(C)]
        nonlinear = dict(nonlinear or {})
        if len(nonlinear) > _lib.PINN_SYSTEM_MAX_NONLINEAR:
            raise ValueError(f"{who}: {len(nonlinear)} nonlinear functions; a system names at most {_lib.PINN_SYSTEM_MAX_NONLINEAR}")
        nl_index: Dict[str, int] = {}
        self._nonlinear: List[Tuple[str, str, object]] = []  # (name, op, source as the descriptor takes it); function k is "nl<k>"
        self._nl_specs: List[Tuple[object, object, object]] = []  # (shift, scale, exponent): a number or (number, parameter name)
        for k, (name, decl) in enumerate(nonlinear.items()):
            if (not isinstance(name, str) or not name.isidentifier() or "_" in name or name in _COORDS or name in index
                    or name in ("sin", "cos") or name in fn_index):
                raise ValueError(f"{who}: nonlinear name {name!r}: an identifier without '_' that is none of x, y, z, t, sin, cos, no "
                                 f"field name ({', '.join(fields)}) and no function name")
            if not isinstance(decl, (tuple, list)) or len(decl) not in (2, 3) or (len(decl) == 3 and not isinstance(decl[2], dict)):
                raise ValueError(f"{who}: nonlinear '{name}': (op, source) or (op, source, {{'shift': .., 'scale': .., 'exponent': ..}})")
            op, source = decl[0], decl[1]
            opts = dict(decl[2]) if len(decl) == 3 else {}
            if op not in _lib.NL_OPS:
                raise ValueError(f"{who}: nonlinear '{name}': unknown operation {op!r} (one of {', '.join(_lib.NL_OPS)})")
            if set(opts) - {"shift", "scale", "exponent"}:
                raise ValueError(f"{who}: nonlinear '{name}': unknown options {sorted(set(opts) - {'shift', 'scale', 'exponent'})} "
                                 "(shift, scale, exponent)")
            if isinstance(source, str) and source in nl_index:
                src: object = f"nl{nl_index[source]}"
            else:
                parsed = None if (isinstance(source, str) and (source in fn_index or source in nonlinear)) else \
                    self._parse_factor(source, index)
                if parsed is None or parsed[0] is None or parsed[1] in ("sin(u)", "cos(u)"):
                    raise ValueError(f"{who}: nonlinear '{name}': source {source!r} is neither a stream of a field ({self._FACTOR_NAMES} "
                                     f"without sin and cos, <field> in {', '.join(fields)}) nor an earlier nonlinear name "
                                     f"({', '.join(nl_index) or 'none so far'}); a coordinate, a known function and a later declaration "
                                     "are no sources")
                c, one, t_order, (axis, order) = parsed
                if order and axis >= dim:
                    raise ValueError(f"{who}: nonlinear '{name}': source '{source}' needs dimension {axis + 1}, the problem has {dim}")
                nt[c] = max(nt[c], t_order)
                nx[c][axis] = max(nx[c][axis], order)
                self._factor_parsed(c, one, nx)
                src = (c, one)
            spec = []
            for key, default in (("shift", 0.0), ("scale", 1.0), ("exponent", 1.0)):
                v = opts.get(key, default)
                if isinstance(v, str):
                    v = (1.0, v)
                if isinstance(v, (tuple, list)):
                    if len(v) != 2 or not isinstance(v[1], str):
                        raise ValueError(f"{who}: nonlinear '{name}': {key} is a number, a parameter name or (number, 'parameter name')")
                    v = (float(v[0]), v[1])
                else:
                    v = float(v)
                spec.append(v)
            nl_index[name] = k
            self._nonlinear.append((name, op, src))
            self._nl_specs.append(tuple(spec))
        for e, eq in enumerate(equations):
            for coef, factors in eq:
                m = len(self._term_coefs)
                factors = (factors,) if isinstance(factors, str) else tuple(factors)
                if len(factors) > _lib.PINN_TERM_MAX_FACTORS:
                    raise ValueError(f"{who}: equation {e}, term {m} has {len(factors)} factors; a term has at most "
                                     f"{_lib.PINN_TERM_MAX_FACTORS}")
                row = []
                for f in factors:
                    if isinstance(f, str) and f in fn_index:  # a known function: a factor like a coordinate
                        row.append(f"fn{fn_index[f]}")
                        continue
                    if isinstance(f, str) and f in nl_index:  # a nonlinear function of the unknowns
                        row.append(f"nl{nl_index[f]}")
                        continue
                    parsed = self._parse_factor(f, index)
                    if parsed is None:
                        raise ValueError(f"{who}: equation {e}, term {m}: unknown factor '{f}' (a coordinate x, y, z, t, or one of "
                                         f"{self._FACTOR_NAMES} with "
                                         f"<field> in {', '.join(fields)}; {self._FACTOR_NOTE})")
                    c, name, t_order, (axis, order) = parsed
                    need = _COORDS[name] if c is None else (axis if order else 0)
                    if need >= dim:
                        raise ValueError(f"{who}: equation {e}, term {m}: factor '{f}' needs dimension {need + 1}, the problem has {dim}")
                    if c is None:
                        row.append(name)
                        continue
                    nt[c] = max(nt[c], t_order)
                    nx[c][axis] = max(nx[c][axis], order)
                    self._factor_parsed(c, name, nx)
                    row.append((c, name))
                if isinstance(coef, (tuple, list)):
                    if len(coef) != 2 or not isinstance(coef[1], str):
                        raise ValueError(f"{who}: equation {e}, term {m}: a coefficient is a number or (scale, 'parameter name')")
                    coef = (float(coef[0]), coef[1])
                else:
                    coef = float(coef)
                self._term_coefs.append(coef)
                self._term_factors.append(tuple(row))
                self._equation_of.append(e)
        for c in range(C):
            try:
                nt[c], nx[c][0] = _pick_stream_set(nt[c], nx[c][0])
            except NotImplementedError:
                raise NotImplementedError(
                    f"{who}: the factors of field '{fields[c]}' need time order {nt[c]} together with order {nx[c][0]} along x, and no "
                    "compiled stream set holds both (time order 2 goes with space order 0 or 2)") from None
        self._nt, self._nx = tuple(nt), tuple(tuple(v) for v in nx)
        E = len(equations)
        w = [1.0] * E if equation_weights is None else [float(v) for v in equation_weights]
        if len(w) != E or any(not (v >= 0.0 and v != float("inf")) for v in w):
            raise ValueError(f"{who}: equation_weights: {E} finite weights >= 0 (got {equation_weights})")
        self._eq_weights = tuple(w)
        # ---- boundary and initial conditions
        bcs = dict(getattr(config, "boundary_conditions", None) or {})
        self._faces: Optional[FaceConditions] = None
        if face_conditions is not None:
            check_face_arguments(who, face_conditions, config)
            self._faces = FaceConditions(who, face_conditions, dim, fields)
            self._bc = ("faces", None)
            n_bc_terms = len(self._faces)
        elif list(bcs) == ["dirichlet"]:
            p = bcs["dirichlet"] or {}
            if p.get("type", "fixed") != "fixed":
                raise NotImplementedError(f"{who}: dirichlet boundary of type '{p.get('type')}': a fixed value on all faces only")
            v = p.get("value", 0.0)
            vals = list(v) if isinstance(v, (list, tuple)) else [v] * C
            if len(vals) != C:
                raise ValueError(f"{who}: dirichlet value {v}: a number or one entry (a number or None) per field ({C})")
            self._bc = ("dirichlet", tuple(None if x is None else float(x) for x in vals))
            n_bc_terms = sum(x is not None for x in vals)
        elif list(bcs) == ["periodic"]:
            self._bc = ("periodic", None)
            n_bc_terms = dim * C
        else:
            raise NotImplementedError(
                f"{who}: boundary conditions {sorted(bcs)}: exactly one of {{'dirichlet': {{'type': 'fixed', 'value': v}}}} on all "
                "faces or {'periodic': {}} (Neumann and Robin faces read derivative streams on the faces: not available)")
        ic_fields = fields if initial_condition_fields is None else tuple(initial_condition_fields)
        for name in ic_fields:
            if name not in index:
                raise ValueError(f"{who}: initial_condition_fields names '{name}', which is none of the fields {fields}")
        if len(set(ic_fields)) != len(ic_fields):
            raise ValueError(f"{who}: initial_condition_fields {ic_fields} repeat")
        self._ic_fields = tuple(index[name] for name in ic_fields)
        # the data terms of `observations` (one per observed field) ride the same chain: they count
        n_data = 0
        if isinstance(observations, dict):
            of = observations.get("fields")
            n_data = C if of is None else (1 if isinstance(of, str) else len(tuple(of)))
        if self._faces is not None:
            if n_data and n_bc_terms + len(self._ic_fields) + n_data > _lib.PINN_FACE_MAX_TERMS:
                raise ValueError(f"{who}: the boundary / initial / data chain has {n_bc_terms + len(self._ic_fields) + n_data} loss terms "
                                 f"({n_bc_terms} boundary + {len(self._ic_fields)} initial + {n_data} data); one pinn_face_losses call "
                                 f"takes at most {_lib.PINN_FACE_MAX_TERMS}")
            check_term_count(who, n_bc_terms, len(self._ic_fields))
        elif n_bc_terms + len(self._ic_fields) + n_data > PINN_MAX_POINT_TERMS:
            raise NotImplementedError(
                f"{who}: the boundary / initial chain has {n_bc_terms + len(self._ic_fields) + n_data} loss terms ({n_bc_terms} boundary + "
                f"{len(self._ic_fields)} initial" + (f" + {n_data} data" if n_data else "") + f"); one pinn_jet_losses call takes at most "
                f"{PINN_MAX_POINT_TERMS}")
        if list(getattr(config, "trainable_parameters", []) or []):
            raise NotImplementedError(f"{who}: trainable parameters (inverse problems) are not covered: the coefficients of a "
                                      "term residual are read by value")
        # ---- learnable parameters: names of config.parameters behind term coefficients and nonlinear entries
        learn = dict(learn or {})
        if len(learn) > _lib.PINN_SYSTEM_MAX_PARAMS:
            raise ValueError(f"{who}: learn names {len(learn)} parameters; a system learns at most {_lib.PINN_SYSTEM_MAX_PARAMS}")
        used = {c[1] for c in self._term_coefs if isinstance(c, tuple)}
        used |= {v[1] for spec in self._nl_specs for v in spec if isinstance(v, tuple)}
        for name, guess in learn.items():
            if not isinstance(name, str) or name not in (getattr(config, "parameters", None) or {}):
                raise ValueError(f"{who}: learn names '{name}', which is not in config.parameters")
            if name not in used:
                raise ValueError(f"{who}: learn names '{name}', which no term coefficient and no nonlinear shift / scale / exponent uses")
            if guess is not None and not (isinstance(guess, (int, float)) and float(guess) == float(guess)
                                          and abs(float(guess)) != float("inf")):
                raise ValueError(f"{who}: learn['{name}'] = {guess!r}: a finite initial guess, or None for the config's value")
        for (name, op, _), spec in zip(self._nonlinear, self._nl_specs):
            if isinstance(spec[2], tuple) and spec[2][1] in learn and op != "pow":
                raise ValueError(f"{who}: nonlinear '{name}': the exponent '{spec[2][1]}' is learnable, which needs the operation 'pow' "
                                 f"(got '{op}': it does not read the exponent)")
        self._learn: Tuple[str, ...] = tuple(learn)
        super().__init__(config)
        self.config.output_dim = C
        if self._training_mode() != "forward" or self.observation_data:
            raise NotImplementedError(f"{who}: data modes and observation data are not covered (forward problems only)")
        # the one (P,) tensor the kernel reads at launch time and the optimiser updates in place, in the order of `learn`
        self.learned: Optional[torch.nn.Parameter] = None
        if self._learn:
            init = [float(self.config.parameters[name]) if learn[name] is None else float(learn[name]) for name in self._learn]
            self.learned = torch.nn.Parameter(torch.tensor(init, dtype=torch.float32, device=self.device))
        self._obs = self._check_observations(who, observations, index)
        for coef in self._term_coefs:
            if isinstance(coef, tuple) and self.get_parameter(coef[1]) is None:
                raise ValueError(f"{who}: coefficient parameter '{coef[1]}' is not in config.parameters")
        for (name, _, _), spec in zip(self._nonlinear, self._nl_specs):
            for v in spec:
                if isinstance(v, tuple) and self.get_parameter(v[1]) is None:
                    raise ValueError(f"{who}: nonlinear '{name}': parameter '{v[1]}' is not in config.parameters")
        self._nl_values: Optional[torch.Tensor] = None
        self._initial_condition_fn = initial_condition_fn
        self._exact_solution_fn = exact_solution_fn
        self._nb, self._ni = int(boundary_points_per_axis), int(initial_points_per_axis)
        self._coef_values: Optional[torch.Tensor] = None
        self._coef_device: Optional[torch.device] = None
        self._descs: Dict[Any, Any] = {}
        self._points: Optional[Tuple[torch.device, Dict[str, Any]]] = None

    def _factor_parsed(self, c: int, name: str, nx: List[List[int]]) -> None:
        """Hook of the constructor's term loop, called for every field factor after its orders went into nx (the space orders per
        field and axis, a list to be changed in place).  Nothing to do here."""

    @staticmethod
    def _parse_factor(f: str, index: Dict[str, int]):
        """(field index | None, one-field factor name, time order, (axis, space order)) of a factor name, or None."""
        if not isinstance(f, str):
            return None
        if f in _COORDS:
            return None, f, 0, (0, 0)
        for fn in ("sin", "cos"):
            if f.startswith(fn + "(") and f.endswith(")") and f[4:-1] in index:
                return index[f[4:-1]], f"{fn}(u)", 0, (0, 0)
        name, _, suffix = f.partition("_")
        if name in index and suffix in _SUFFIX and ("_" in f) == bool(suffix):
            one, t_order, axis_order = _SUFFIX[suffix]
            return index[name], one, t_order, axis_order
        return None

    # ---------------------------------------------------------------- coefficients and descriptors
    @property
    def n_fields(self) -> int:
        return len(self.fields)

    @property
    def n_equations(self) -> int:
        return len(self._eq_weights)

    def _stored(self, v):
        """The number the kernel is handed for a coefficient or a nonlinear entry: the value, or for a learnable entry its SCALE
        (the kernel multiplies it with the parameter it reads from `learned`)."""
        if not isinstance(v, tuple):
            return v
        return v[0] if v[1] in self._learn else v[0] * float(self.get_parameter(v[1], required=True))

    def _coefficients(self):
        return tuple(self._stored(c) for c in self._term_coefs)

    def get_parameter(self, name: str, default=None, required: bool = False):
        """`PDEBase.get_parameter`; a learnable name returns its CURRENT value (a host read of `learned`)."""
        learn = getattr(self, "_learn", ())
        if name in learn and getattr(self, "learned", None) is not None:
            return float(self.learned.detach()[learn.index(name)].cpu())
        return super().get_parameter(name, default, required)

    def trainable_parameters_iter(self):
        """The learnable parameter tensor, so that `PDETrainer`'s optimiser holds it beside the network's."""
        return iter([self.learned]) if self._learn else super().trainable_parameters_iter()

    def learned_values(self) -> Dict[str, float]:
        """{name: current value} of the learnable parameters, in the order of `learn`."""
        if not self._learn:
            return {}
        vals = self.learned.detach().cpu().tolist()
        return {name: float(v) for name, v in zip(self._learn, vals)}

    def _param_index(self, v) -> int:
        return self._learn.index(v[1]) if isinstance(v, tuple) and v[1] in self._learn else -1

    def _check_observations(self, who: str, obs, index: Dict[str, int]):
        """The `observations` keyword as device tensors: {"x": (n, dim), "t": (n, 1), "u": (k, n) one contiguous row per observed
        field, "fields": their indices}, or None."""
        if obs is None:
            return None
        if not isinstance(obs, dict) or set(obs) - {"x", "t", "u", "fields"} or not {"x", "t", "u"} <= set(obs):
            raise ValueError(f"{who}: observations is a mapping with 'x': (n, {self.dimension}), 't': (n, 1), 'u': (n, k) and "
                             "optionally 'fields'")
        names = self.fields if obs.get("fields") is None else ((obs["fields"],) if isinstance(obs["fields"], str) else tuple(obs["fields"]))
        for name in names:
            if name not in index:
                raise ValueError(f"{who}: observations names the field '{name}', which is none of the fields {self.fields}")
        if not names or len(set(names)) != len(names):
            raise ValueError(f"{who}: observations['fields'] {names}: at least one field, none twice")
        dev = self.device
        x, t, u = (torch.as_tensor(obs[k], dtype=torch.float32).detach() for k in ("x", "t", "u"))
        n = x.shape[0] if x.dim() == 2 else -1
        if x.dim() != 2 or x.shape[1] != self.dimension or n < 1:
            raise ValueError(f"{who}: observations['x'] has shape {tuple(x.shape)}, expected (n, {self.dimension}) with n >= 1")
        if tuple(t.shape) != (n, 1):
            raise ValueError(f"{who}: observations['t'] has shape {tuple(t.shape)}, expected ({n}, 1)")
        if tuple(u.shape) != (n, len(names)):
            raise ValueError(f"{who}: observations['u'] has shape {tuple(u.shape)}, expected ({n}, {len(names)}): one column per "
                             f"observed field {names}")
        if not (bool(torch.isfinite(x).all()) and bool(torch.isfinite(t).all()) and bool(torch.isfinite(u).all())):
            raise ValueError(f"{who}: observations hold NaN or inf")
        return {"x": x.to(dev).contiguous(), "t": t.to(dev).contiguous(), "u": u.t().contiguous().to(dev),
                "fields": tuple(index[name] for name in names), "n": n}

    def _has_trainable_coefficients(self) -> bool:
        return False

    @property
    def coef_values(self) -> torch.Tensor:
        """The c_m as float32 on the PDE's device, one per term, built once: what the kernel reads at launch time."""
        dev = torch.device(self.device)  # the REQUESTED device is remembered beside the tensor (see TermPDE.coef_values)
        if self._coef_values is None or self._coef_device != dev:
            self._coef_values = torch.tensor([float(c) for c in self._coefficients()], dtype=torch.float32, device=dev).reshape(-1)
            self._nl_values = torch.tensor(
                [[self._stored(v) for v in spec]
                 for spec in self._nl_specs], dtype=torch.float32, device=dev).reshape(len(self._nl_specs), 3)
            if self.learned is not None and self.learned.device != self._coef_values.device:
                self.learned.data = self.learned.data.to(self._coef_values.device)  # the same Parameter object: an optimiser keeps it
            self._coef_device = dev
            self._descs = {}
        return self._coef_values

    @property
    def nl_values(self) -> torch.Tensor:
        """{shift, scale, exponent} of every nonlinear function as a (K, 3) float32 tensor on the PDE's device, built once beside
        `coef_values`: what the kernel reads at launch time."""
        self.coef_values
        return self._nl_values

    def _fn_desc(self, loss: str, delta: float) -> "_E.FnSystemTermDesc":
        """The descriptor of a problem with functions: a `FnSystemTermDesc` (here with all pair orders 0); with nonlinear
        functions of the unknowns an `NlSystemTermDesc`."""
        cv = self.coef_values
        key = (loss, float(delta))
        if key not in self._descs and self._learn:  # an inverse problem: the maps from terms and entries to `learned`
            nl = [(op, src, 0.0, 1.0, 1.0) for _, op, src in self._nonlinear]
            self._descs[key] = _E.InvSystemTermDesc(
                self._term_factors, self._equation_of, cv, self.dimension, self.n_fields, self.n_equations, self._nt, self._nx,
                getattr(self, "_pair", None), [g for _, g in self._functions], nl, self._eq_weights, loss, delta,
                [name for name, _ in self._functions], [name for name, _, _ in self._nonlinear], self.nl_values, self.learned,
                [self._param_index(c) for c in self._term_coefs], [[self._param_index(v) for v in spec] for spec in self._nl_specs])
        if key not in self._descs and self._nonlinear:
            nl = [(op, src, 0.0, 1.0, 1.0) for _, op, src in self._nonlinear]  # the numbers are in nl_values
            self._descs[key] = _E.NlSystemTermDesc(self._term_factors, self._equation_of, cv, self.dimension, self.n_fields,
                                                   self.n_equations, self._nt, self._nx, getattr(self, "_pair", None),
                                                   [g for _, g in self._functions], nl, self._eq_weights, loss, delta,
                                                   [name for name, _ in self._functions], [name for name, _, _ in self._nonlinear],
                                                   self.nl_values)
        if key not in self._descs:
            self._descs[key] = _E.FnSystemTermDesc(self._term_factors, self._equation_of, cv, self.dimension, self.n_fields,
                                                   self.n_equations, self._nt, self._nx, getattr(self, "_pair", None),
                                                   [g for _, g in self._functions], self._eq_weights, loss, delta,
                                                   [name for name, _ in self._functions])
        return self._descs[key]

    def _term_desc(self, loss: str, delta: float) -> "_E.SystemTermDesc":
        if self._functions or self._nonlinear or self._learn:
            return self._fn_desc(loss, delta)
        cv = self.coef_values
        key = (loss, float(delta))
        if key not in self._descs:
            self._descs[key] = _E.SystemTermDesc(self._term_factors, self._equation_of, cv, self.dimension, self.n_fields,
                                                 self.n_equations, self._nt, self._nx, self._eq_weights, loss, delta)
        return self._descs[key]

    def _pde_desc(self):
        return self._term_desc(self._loss_function_name(), self._huber_delta())

    def _pde_desc_l1(self):
        return self._term_desc("mae", 1.0)

    def exact_solution(self, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        if self._exact_solution_fn is None:
            raise NotImplementedError(f"{type(self).__name__}: no exact_solution_fn was given")
        u = self._exact_solution_fn(x, t)
        if u.dim() != 2 or u.shape[1] != self.n_fields:
            raise ValueError(f"{type(self).__name__}: exact_solution_fn returned {tuple(u.shape)}, expected (n, {self.n_fields})")
        return u

    def validate(self, model, num_points: int = 1000) -> Dict[str, float]:
        """`PDEBase.validate` over all fields, plus "relative_l2_error" = ||u_pred - u_exact|| / ||u_exact|| over all of them."""
        x, t = self.generate_collocation_points(num_points)
        with torch.no_grad():
            u_pred = model(torch.cat([x, t], dim=1))
        exact = self.exact_solution(x, t).to(u_pred.dtype)
        err = torch.abs(u_pred - exact)
        return {"l2_error": torch.mean(err**2).item(), "max_error": torch.max(err).item(), "mean_error": torch.mean(err).item(),
                "relative_l2_error": (torch.linalg.norm(err) / torch.linalg.norm(exact)).item()}

    def _check_model(self, model) -> None:
        C = getattr(getattr(model, "model", model), "output_dim", None)
        if C is not None and int(C) != self.n_fields:
            raise ValueError(f"{type(self).__name__}: {self.n_fields} fields {self.fields} need a model with output_dim = {self.n_fields} "
                             f"(this one has {C})")

    def compute_residual(self, model, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """(N, E) residuals with a grad_fn towards the network parameters."""
        self._check_model(model)
        return super().compute_residual(model, x, t)

    # ---------------------------------------------------------------- fixed evaluation points
    def _system_points(self) -> Dict[str, Any]:
        """`box_points` of the problem, built once per device, with u0 (n_ic, number of initial fields) the initial targets and,
        under Dirichlet faces, ub[c] (n_bc,) the constant target of field c (None where the field has no boundary term)."""
        dev = torch.device(self.device)
        if self._points is not None and self._points[0] == dev:
            return self._points[1]
        pts = box_points(self.domain, self.time_domain, self.dimension, self._nb, self._ni, dev)
        if self._ic_fields:
            with torch.no_grad():
                u0 = self._initial_condition_fn(pts["xi"])
        else:  # a problem known only from data: no initial term, the function is not called
            u0 = torch.zeros((pts["n_ic"], 0), dtype=torch.float32, device=dev)
        u0 = (u0.reshape(-1, 1) if u0.dim() == 1 else u0).float()
        if tuple(u0.shape) != (pts["n_ic"], len(self._ic_fields)):
            raise ValueError(f"{type(self).__name__}: initial_condition_fn returned {tuple(u0.shape)} for {pts['n_ic']} points, expected "
                             f"({pts['n_ic']}, {len(self._ic_fields)})")
        pts["u0"] = u0.t().contiguous().to(dev)  # (fields, n_ic): one contiguous target per initial field
        if self._bc[0] == "dirichlet":
            pts["ub"] = [None if v is None else torch.full((pts["n_bc"],), v, dtype=torch.float32, device=dev) for v in self._bc[1]]
        if self._faces is not None:
            pts["face_targets"] = self._faces.targets(type(self).__name__, pts)
        self._points = (dev, pts)
        return pts

    # ---------------------------------------------------------------- losses
    def compute_loss(self, model, x: torch.Tensor, t: torch.Tensor, n_total: Optional[int] = None,
                     aux_scale: float = 1.0) -> Dict[str, torch.Tensor]:
        """residual = sum_e omega_e mean l(r_e) (the chain behind `engine.residual_loss_grad`); boundary and initial: sums over
        the fields of the means on the fixed points, from ONE (n, C) forward of the model (C component launches, differentiable
        through `JetFunction`); then `_compose_losses`' tail."""
        self._check_model(model)
        dev = self.device
        residual_loss = self._residual_loss(model, x, t, n_total)
        P = self._system_points()
        u = model(torch.cat([P["x"], P["t"]], dim=1))
        nbc, nf = P["n_bc"], P["n_face"]
        boundary_loss = torch.zeros((), device=dev)
        if self._faces is not None:
            boundary_loss = self._faces.boundary_loss(self, model, P, P["face_targets"], u)
        for c in range(self.n_fields):
            if self._faces is not None:
                break
            if self._bc[0] == "dirichlet":
                if P["ub"][c] is not None:
                    boundary_loss = boundary_loss + self._apply_loss_fn(u[:nbc, c] - P["ub"][c])
            else:
                for a in range(self.dimension):
                    lo = 2 * a * nf
                    boundary_loss = boundary_loss + self._apply_loss_fn(u[lo : lo + nf, c] - u[lo + nf : lo + 2 * nf, c])
        initial_loss = torch.zeros((), device=dev)
        for k, c in enumerate(self._ic_fields):
            initial_loss = initial_loss + self._apply_loss_fn(u[nbc:, c] - P["u0"][k])
        zero = torch.zeros((), device=dev)
        data_loss = zero
        if self._obs is not None:  # sum over the observed fields of mean l(u_c(obs) - target_c); the other fields stay hidden
            uo = model(torch.cat([self._obs["x"], self._obs["t"]], dim=1))
            for k, c in enumerate(self._obs["fields"]):
                data_loss = data_loss + self._apply_loss_fn(uo[:, c] - self._obs["u"][k])
        return self._compose_losses(residual_loss, boundary_loss, initial_loss, zero, data_loss, aux_scale)

    def _residual_loss(self, model, x: torch.Tensor, t: torch.Tensor, n_total: Optional[int] = None) -> torch.Tensor:
        """`PDEBase._residual_loss`; with `learn` the node also carries d loss / d learned, from the same chain
        (`engine.ResidualLossParamFunction`)."""
        if not self._learn:
            return super()._residual_loss(model, x, t, n_total)
        if self._causal_weighting() is not None:
            raise NotImplementedError(f"{type(self).__name__}: causal weighting with learn is not covered")
        _jets_of(model)
        self._prepare_model(model)
        prog = model.program()
        x = x.detach().to(self.device)
        t = t.detach().to(self.device)
        n = int(n_total) if n_total is not None else x.shape[0]
        return _E.ResidualLossParamFunction.apply(prog, self._pde_desc(), x, t, n, self.learned, *prog.tensors)

    def _manual_chain(self, n_batch: int) -> Dict[str, Any]:
        """`compute_loss`' boundary / initial part as data for the launch list.  "components" = C: the value rows of the C
        component forwards on the fixed points are stacked as a (C, n) block, the loss terms name their field as the stream, and
        row c of the cotangent block feeds component c's reverse launch.  Boundary terms in the order of `compute_loss`."""
        P = self._system_points()
        lw = self._loss_weights()
        bw, iw = (lw.get("boundary", 10.0), lw.get("initial", 10.0)) if lw else (10.0, 10.0)
        nbc, nf = P["n_bc"], P["n_face"]
        obs = self._obs
        xs, ts, n_fixed = P["x"], P["t"], P["x"].shape[0]
        dw = 1.0
        if obs is not None:  # the observation points behind the fixed ones; one loss term per observed field, its field the stream
            xs, ts = torch.cat([P["x"], obs["x"]], 0).contiguous(), torch.cat([P["t"], obs["t"]], 0).contiguous()
            dw = float(self._data_loss_weight(1.0))
        if self._faces is not None:  # no "terms": "face" holds the jet launches and the pinn_face_losses table
            initial = [(c, P["u0"][k], float(iw)) for k, c in enumerate(self._ic_fields)]
            face = self._faces.chain(P, P["face_targets"], float(bw), initial)
            out = {"x": xs, "t": ts, "nt": 0, "nx": 0, "terms": [], "n_bc": len(self._faces), "components": self.n_fields, "face": face}
            if obs is not None:
                # the value launch of an observed field is extended over the observation points (a field without one gets a launch
                # over them alone); the data terms come after the initial ones
                launches = list(face["launches"])
                for k, c in enumerate(obs["fields"]):
                    hit = [i for i, (lo, hi, nt, nx, axis, comp) in enumerate(launches)
                           if (lo, nt, nx, axis, comp) == (0, 0, 0, 0, c) and hi >= n_fixed]
                    if hit:
                        launches[hit[0]] = (0, n_fixed + obs["n"], 0, 0, 0, c)
                        where = (hit[0], 0, n_fixed)
                    else:
                        launches.append((n_fixed, n_fixed + obs["n"], 0, 0, 0, c))
                        where = (len(launches) - 1, 0, 0)
                    face["terms"].append({"n": obs["n"], "alpha": 1.0, "beta": 0.0, "target": obs["u"][k], "weight": dw, "value": where})
                face["launches"] = launches
                out["n_data"] = len(obs["fields"])
            return out
        terms = []
        for c in range(self.n_fields):
            if self._bc[0] == "dirichlet":
                if P["ub"][c] is not None:
                    terms.append((0, nbc, c, 0, P["ub"][c], float(bw)))
            else:
                terms += [(2 * a * nf, 2 * a * nf + nf, c, nf, None, float(bw)) for a in range(self.dimension)]
        n_bc_terms = len(terms)
        for k, c in enumerate(self._ic_fields):
            terms.append((nbc, nbc + P["n_ic"], c, 0, P["u0"][k], float(iw)))
        out = {"x": xs, "t": ts, "nt": 0, "nx": 0, "terms": terms, "n_bc": n_bc_terms, "components": self.n_fields}
        if obs is not None:
            terms += [(n_fixed, n_fixed + obs["n"], c, 0, obs["u"][k], dw) for k, c in enumerate(obs["fields"])]
            out["n_data"] = len(obs["fields"])
        return out
