"""Per-face boundary conditions of the term PDEs (`face_conditions=` of `TermPDEnD`, `TermPDEMixed`, `TermPDESystem`).

A face of the box is named by axis and side.  The keys of `face_conditions`, from the least to the most specific:

    "default"                  every face
    "x", "y", "z"              both faces of that axis
    "x_lo", "x_hi", "y_lo" ..  one face

A face name overrides an axis name, an axis name overrides "default".  Every face must resolve to a spec or to an explicit
None (no condition on that face).  A spec is a dict:

    {"type": "dirichlet", "value": v}                        u = v
    {"type": "neumann", "value": v}                          du/dn = v
    {"type": "robin", "alpha": a, "beta": b, "value": v}     a u + b du/dn = v   (a, b finite, not both zero)
    {"type": "periodic", "derivative": False}                axis or default level only: point k of the low face paired with
                                                             point k of the high one; "derivative": True pairs du/dx_a too

d/dn is the OUTWARD normal derivative: -d/dx_a on the low face, +d/dx_a on the high face.  `value` (default 0) is a number or a
callable value(x: (n, dim), t: (n, 1)) -> (n,), evaluated once, under no_grad, on the face's fixed points.

In a system the value under a key is a spec (every field) or a mapping {field name: spec | None}; a field the mapping does not
list follows the next less specific key.  A spec is told from a mapping by its key "type" holding a str.  No condition couples
fields.

Each (face, field) with a condition is one loss term, the mean of l(d) over the face's points; a periodic axis is one paired
term per field, and one more with "derivative": True.  The boundary loss is the SUM of the terms (as the periodic config form
sums over axes and the system form over fields): {"default": {"type": "dirichlet", "value": v}} gives 2 dim times the boundary
loss of the config form {"dirichlet": {"type": "fixed", "value": v}}, which is one mean over all faces.

On the launch list every term is one entry of a `pinn_face_losses` table,
    d_i = alpha (A[i] - A'[i]) + beta (B[i] - B'[i]) - T_i,
A a segment of the value row of the field's (0, 0) launch on all fixed points, B a segment of the derivative row of one launch
per (field, axis) over that axis's two faces: the set (1, 1) on axis 0 (the ABI has no space-only set there), (0, 1) along an
axis >= 1.
"""

from __future__ import annotations

import math
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from .. import _lib

PINN_FACE_MAX_TERMS = _lib.PINN_FACE_MAX_TERMS
_AXES = "xyz"
_SPEC_KEYS = {"dirichlet": {"type", "value"}, "neumann": {"type", "value"}, "robin": {"type", "value", "alpha", "beta"},
              "periodic": {"type", "derivative"}}


class FaceTerm(NamedTuple):
    """One boundary loss term.  side 0 / 1: d = alpha u + beta du/dx_axis - value on that face (beta carries the sign of the
    outward normal); side None: a periodic pair, d = alpha (u_lo - u_hi) + beta (du/dx_axis_lo - du/dx_axis_hi)."""
    field: int
    axis: int
    side: Optional[int]
    alpha: float
    beta: float
    value: Union[float, Callable]


def _is_spec(v) -> bool:
    return isinstance(v, dict) and isinstance(v.get("type"), str)


def _check_spec(who: str, key: str, spec: Dict[str, Any]) -> None:
    kind = spec["type"]
    if kind not in _SPEC_KEYS:
        raise ValueError(f"{who}: face_conditions['{key}']: type '{kind}' (one of dirichlet, neumann, robin, periodic)")
    extra = sorted(set(spec) - _SPEC_KEYS[kind])
    if extra:
        raise ValueError(f"{who}: face_conditions['{key}']: a {kind} spec has the keys {sorted(_SPEC_KEYS[kind])}, not {extra}")
    if kind == "periodic":
        if not isinstance(spec.get("derivative", False), bool):
            raise ValueError(f"{who}: face_conditions['{key}']: 'derivative' is True or False")
        return
    v = spec.get("value", 0.0)
    if not callable(v) and not (isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(float(v))):
        raise ValueError(f"{who}: face_conditions['{key}']: value {v!r}: a finite number or a callable value(x, t) -> (n,)")
    if kind == "robin":
        for name in ("alpha", "beta"):
            c = spec.get(name)
            if not (isinstance(c, (int, float)) and not isinstance(c, bool) and math.isfinite(float(c))):
                raise ValueError(f"{who}: face_conditions['{key}']: robin needs a finite float '{name}' (got {c!r})")
        if float(spec["alpha"]) == 0.0 and float(spec["beta"]) == 0.0:
            raise ValueError(f"{who}: face_conditions['{key}']: robin with alpha = beta = 0 is no condition")


class FaceConditions:
    """`face_conditions` resolved for a box in `dim` dimensions and the fields `fields` (None: one unnamed field, specs only).
    `terms`: the boundary loss terms, field by field, axis by axis, low face before high face; a periodic axis gives its paired
    value term and then, with "derivative": True, its paired derivative term."""

    def __init__(self, who: str, face_conditions: Dict[str, Any], dim: int, fields: Optional[Sequence[str]] = None):
        if not isinstance(face_conditions, dict):
            raise TypeError(f"{who}: face_conditions is a dict of face names to specs (got {type(face_conditions).__name__})")
        self.dim = int(dim)
        names = tuple(fields) if fields is not None else (None,)
        axes = _AXES[: self.dim]
        face_keys = {f"{ax}_{s}": (a, k) for a, ax in enumerate(axes) for k, s in enumerate(("lo", "hi"))}
        for key, val in face_conditions.items():
            ax = key.split("_")[0] if isinstance(key, str) else ""
            if key != "default" and key not in axes and key not in face_keys:
                if ax in _AXES and ax not in axes and key in (ax, ax + "_lo", ax + "_hi"):
                    raise ValueError(f"{who}: face_conditions['{key}'] names axis '{ax}', the problem has dimension {self.dim} "
                                     f"(axes {', '.join(axes)})")
                raise ValueError(f"{who}: face_conditions key {key!r}: 'default', an axis ({', '.join(axes)}) or a face "
                                 f"({', '.join(face_keys)})")
            if val is None or _is_spec(val):
                entries = [(key, val)]
            elif isinstance(val, dict) and fields is not None:
                for name in val:
                    if name not in names:
                        raise ValueError(f"{who}: face_conditions['{key}'] names '{name}', which is none of the fields {names} "
                                         "(a spec has a key 'type' holding a str)")
                entries = [(f"{key}']['{name}", v) for name, v in val.items()]
            else:
                raise ValueError(f"{who}: face_conditions['{key}']: a spec {{'type': ...}} or None"
                                 + (" or a mapping {field name: spec | None}" if fields is not None else ""))
            for label, spec in entries:
                if spec is None:
                    continue
                if not _is_spec(spec):
                    raise ValueError(f"{who}: face_conditions['{label}']: a spec {{'type': ...}} or None")
                _check_spec(who, label, spec)
                if spec["type"] == "periodic" and key in face_keys:
                    raise ValueError(f"{who}: face_conditions['{label}']: periodic pairs the two faces of an axis: give it for the "
                                     f"axis ('{key.split('_')[0]}') or as 'default', not for a single face")
        self.terms: List[FaceTerm] = []
        for c, name in enumerate(names):
            for a, ax in enumerate(axes):
                specs = [self._resolve(who, face_conditions, name, ax, s) for s in ("lo", "hi")]
                periodic = [sp is not None and sp["type"] == "periodic" for sp in specs]
                if any(periodic):
                    if not all(periodic) or specs[0] is not specs[1]:
                        raise ValueError(f"{who}: axis '{ax}'" + (f", field '{name}'" if name else "") + " is periodic on one face and "
                                         "overridden on the other: periodic pairs both faces of an axis")
                    self.terms.append(FaceTerm(c, a, None, 1.0, 0.0, 0.0))
                    if specs[0].get("derivative", False):
                        self.terms.append(FaceTerm(c, a, None, 0.0, 1.0, 0.0))
                    continue
                for side, sp in enumerate(specs):
                    if sp is None:
                        continue
                    normal = -1.0 if side == 0 else 1.0
                    kind, value = sp["type"], sp.get("value", 0.0)
                    value = value if callable(value) else float(value)
                    if kind == "dirichlet":
                        self.terms.append(FaceTerm(c, a, side, 1.0, 0.0, value))
                    elif kind == "neumann":
                        self.terms.append(FaceTerm(c, a, side, 0.0, normal, value))
                    else:
                        self.terms.append(FaceTerm(c, a, side, float(sp["alpha"]), normal * float(sp["beta"]), value))

    @staticmethod
    def _resolve(who: str, fc: Dict[str, Any], name: Optional[str], ax: str, side: str):
        """The spec (or None) of one face for one field: face name over axis name over "default"."""
        for key in (f"{ax}_{side}", ax, "default"):
            if key not in fc:
                continue
            val = fc[key]
            if val is None or _is_spec(val):
                return val
            if name in val:  # a mapping: a field it does not list follows the next less specific key
                return val[name]
        raise ValueError(f"{who}: face_conditions gives face '{ax}_{side}'" + (f" of field '{name}'" if name else "") + " neither a spec "
                         "nor None (add the face, its axis or 'default')")

    def __len__(self) -> int:
        return len(self.terms)

    # ---------------------------------------------------------------- fixed points
    def targets(self, who: str, P: Dict[str, Any]) -> List[Union[float, torch.Tensor]]:
        """The target of every term on the fixed points `P` (`box_points`): the number, or the callable's values on the face."""
        nf, out = P["n_face"], []
        for k, tm in enumerate(self.terms):
            if not callable(tm.value):
                out.append(float(tm.value))
                continue
            lo = (2 * tm.axis + tm.side) * nf
            with torch.no_grad():
                v = torch.as_tensor(tm.value(P["x"][lo : lo + nf], P["t"][lo : lo + nf]))
            v = v.reshape(-1).float().contiguous()
            if v.shape[0] != nf:
                raise ValueError(f"{who}: the value callable of face '{_AXES[tm.axis]}_{('lo', 'hi')[tm.side]}' returned {v.shape[0]} values "
                                 f"for {nf} points")
            out.append(v.to(P["x"].device))
        return out

    def _deriv_launches(self) -> List[Tuple[int, int]]:
        """The (field, axis) pairs some term reads du/dx_axis of, in term order."""
        seen: List[Tuple[int, int]] = []
        for tm in self.terms:
            if tm.beta != 0.0 and (tm.field, tm.axis) not in seen:
                seen.append((tm.field, tm.axis))
        return seen

    @staticmethod
    def _deriv_set(axis: int) -> Tuple[int, int, int]:
        """(nt, nx, row of du/dx_axis) of the launch that gives du/dx_axis."""
        return (1, 1, 2) if axis == 0 else (0, 1, 1)

    # ---------------------------------------------------------------- autograd form
    def boundary_loss(self, pde, model, P: Dict[str, Any], targets, u: torch.Tensor) -> torch.Tensor:
        """The sum of the boundary terms in torch ops.  u: (n, C) values of the model on the fixed points; du/dx_a on the two
        faces of an axis from `model.jets(..., axis=a, component=c)` (differentiable through `JetFunction`)."""
        nf = P["n_face"]
        deriv: Dict[Tuple[int, int], torch.Tensor] = {}
        for c, a in self._deriv_launches():
            nt, nx, row = self._deriv_set(a)
            lo = 2 * a * nf
            deriv[(c, a)] = model.jets(P["x"][lo : lo + 2 * nf], P["t"][lo : lo + 2 * nf], nt, nx, component=c, axis=a)[row]
        total = torch.zeros((), device=u.device)
        for tm, tg in zip(self.terms, targets):
            lo = 2 * tm.axis * nf
            d = None
            if tm.side is None:
                if tm.alpha != 0.0:
                    d = tm.alpha * (u[lo : lo + nf, tm.field] - u[lo + nf : lo + 2 * nf, tm.field])
                if tm.beta != 0.0:
                    g = deriv[(tm.field, tm.axis)]
                    e = tm.beta * (g[:nf] - g[nf:])
                    d = e if d is None else d + e
            else:
                s = tm.side * nf
                if tm.alpha != 0.0:
                    d = tm.alpha * u[lo + s : lo + s + nf, tm.field]
                if tm.beta != 0.0:
                    e = tm.beta * deriv[(tm.field, tm.axis)][s : s + nf]
                    d = e if d is None else d + e
                d = d - tg
            total = total + pde._apply_loss_fn(d)
        return total

    # ---------------------------------------------------------------- launch-list form
    def chain(self, P: Dict[str, Any], targets, boundary_weight: float,
              initial_terms: Sequence[Tuple[int, torch.Tensor, float]]) -> Dict[str, Any]:
        """The "face" entry of a `_manual_chain` description.  "launches": the forward (and, in the same order, reverse) jet
        launches as (lo, hi, nt, nx, axis, component) over the fixed points [lo, hi); "terms": the `pinn_face_losses` table
        with every segment as (launch, row, first point within the launch) instead of an offset in floats (the trainer lays the
        launches out in one buffer); the boundary terms first, then `initial_terms` = (field, target, weight) on the initial
        points."""
        nf, nbc, nic = P["n_face"], P["n_bc"], P["n_ic"]
        n = nbc + nic
        launches: List[Tuple[int, int, int, int, int, int]] = []
        value_of: Dict[int, int] = {}
        for c in [tm.field for tm in self.terms if tm.alpha != 0.0] + [c for c, _, _ in initial_terms]:
            if c not in value_of:
                value_of[c] = len(launches)
                launches.append((0, n, 0, 0, 0, c))
        deriv_of: Dict[Tuple[int, int], int] = {}
        for c, a in self._deriv_launches():
            nt, nx, _ = self._deriv_set(a)
            deriv_of[(c, a)] = len(launches)
            launches.append((2 * a * nf, 2 * a * nf + 2 * nf, nt, nx, a, c))
        table = []
        for tm, tg in zip(self.terms, targets):
            lo = 2 * tm.axis * nf
            e: Dict[str, Any] = {"n": nf, "alpha": tm.alpha, "beta": tm.beta, "target": tg, "weight": float(boundary_weight)}
            s = 0 if tm.side is None else tm.side * nf
            if tm.alpha != 0.0:
                e["value"] = (value_of[tm.field], 0, lo + s)
                if tm.side is None:
                    e["value_pair"] = (value_of[tm.field], 0, lo + nf)
            if tm.beta != 0.0:
                row = self._deriv_set(tm.axis)[2]
                e["deriv"] = (deriv_of[(tm.field, tm.axis)], row, s)
                if tm.side is None:
                    e["deriv_pair"] = (deriv_of[(tm.field, tm.axis)], row, nf)
            table.append(e)
        for c, tg, w in initial_terms:
            table.append({"n": nic, "alpha": 1.0, "beta": 0.0, "target": tg, "weight": float(w), "value": (value_of[c], 0, nbc)})
        return {"launches": launches, "terms": table}


def check_face_arguments(who: str, face_conditions, config) -> None:
    """`face_conditions` replaces `config.boundary_conditions`: the two together are refused."""
    if dict(getattr(config, "boundary_conditions", None) or {}):
        raise ValueError(f"{who}: face_conditions and config.boundary_conditions "
                         f"{sorted(dict(config.boundary_conditions))} are both given: with face_conditions the config's must be empty")


def check_term_count(who: str, n_boundary: int, n_initial: int) -> None:
    if n_boundary + n_initial > PINN_FACE_MAX_TERMS:
        raise ValueError(f"{who}: the boundary / initial chain has {n_boundary + n_initial} loss terms ({n_boundary} boundary + "
                         f"{n_initial} initial); one pinn_face_losses call takes at most {PINN_FACE_MAX_TERMS}")
