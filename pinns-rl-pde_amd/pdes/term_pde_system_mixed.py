"""`TermPDESystemMixed`: `TermPDESystem` with mixed derivatives (`<field>_xy`) — vector PDEs with a grad-div term.

Linear elasticity, mu Lap(u) + (lambda + mu) grad(div u), names v_xy in the u-equation and u_xy in the v-equation; so do
elastic waves, the viscous terms of compressible flow, poroelasticity and curl-curl Maxwell.  The two ingredients exist
separately: a field of a system is a component launch, and a mixed derivative of one field is the polarisation of
`TermPDEMixed`,

    u_ab = (P_2 - u_aa - u_bb) / 2,   P_2 = (d_a + d_b)^2 u,

with P_2 the order-2 stream of a jet launch along e_a + e_b.  Both are properties of the launch descriptor and compose: naming
"<field>_ab" adds ONE component launch of that field along e_a + e_b on the set (0, 2) and raises the field's orders along a and
b to at least 2.  `pinn_term_residual_system_mixed` derives u_ab per field inside the element-wise kernel and sends the
cotangents back through the transposed map, one block per launch.  Everything else — constructor, fixed points, boundary and
initial handling (config form and `face_conditions`), equation weights, `validate`, the launch list, the captured step, the
flat L-BFGS closure, the refusals — is `TermPDESystem`'s.

Not available: mixed space-time derivatives ("<field>_xt"), third-order mixed derivatives ("<field>_xxy"), "<field>_xxyy"-type
factors and orders above two along y and z ("<field>_yyy").
"""

from __future__ import annotations

from typing import Dict, List

from .. import engine as _E
from .term_pde_system import TermPDESystem

_PAIR_SUFFIX = {"xy": ("u_xy", 0), "xz": ("u_xz", 1), "yz": ("u_yz", 2)}  # suffix -> (the one-field factor name, pair index)
_PAIR_AXES = ((0, 1), (0, 2), (1, 2))


class TermPDESystemMixed(TermPDESystem):
    """`TermPDESystemMixed(config, fields, equations, initial_condition_fn, ...)`: `TermPDESystem`'s constructor for
    `config.dimension` 2 or 3.

    The factor names are `TermPDESystem`'s plus "<field>_xy", "<field>_xz", "<field>_yz" (the z names need dimension 3).

    Linear elasticity in 2-D (Navier-Cauchy with a damping term), fields (u, v), a = lambda + mu:
        TermPDESystemMixed(cfg, ("u", "v"),
                           [[(1.0, ("u_t",)), (-mu, ("u_xx",)), (-mu, ("u_yy",)), (-a, ("u_xx",)), (-a, ("v_xy",))],
                            [(1.0, ("v_t",)), (-mu, ("v_xx",)), (-mu, ("v_yy",)), (-a, ("u_xy",)), (-a, ("v_yy",))]],
                           initial_condition_fn)
    """

    KIND = "term_system_mixed"  # not a `_lib.PDE` kind: the descriptor is a `MixedSystemTermDesc`
    _FACTOR_NAMES = TermPDESystem._FACTOR_NAMES + ", <field>_xy, _xz, _yz"
    _FACTOR_NOTE = ("mixed space-time derivatives (<field>_xt), third-order mixed derivatives (<field>_xxy, _xyy), <field>_xxyy-type "
                    "factors and orders above two along y and z (<field>_yyy) are not available")

    def __init__(self, config, fields, *args, **kwargs):
        dim = int(getattr(config, "dimension", 1))
        if dim not in (2, 3):
            raise NotImplementedError(f"{type(self).__name__}: dimension {dim}: two or three space dimensions (TermPDESystem runs "
                                      "1-D systems)")
        n = 1 if isinstance(fields, str) else len(tuple(fields))
        self._pair_rows: List[List[int]] = [[0, 0, 0] for _ in range(n)]
        super().__init__(config, fields, *args, **kwargs)
        self._pair = tuple(tuple(row) for row in self._pair_rows)

    @staticmethod
    def _parse_factor(f: str, index: Dict[str, int]):
        """`TermPDESystem._parse_factor`, and "<field>_ab" as (field, "u_ab", 0, (b, 2)): the order 2 along the pair's second
        axis goes through the constructor's own checks, `_factor_parsed` adds the first axis and the pair."""
        parsed = TermPDESystem._parse_factor(f, index)
        if parsed is None and isinstance(f, str):
            name, _, suffix = f.partition("_")
            if name in index and suffix in _PAIR_SUFFIX:
                one, k = _PAIR_SUFFIX[suffix]
                return index[name], one, 0, (_PAIR_AXES[k][1], 2)
        return parsed

    def _factor_parsed(self, c: int, name: str, nx: List[List[int]]) -> None:
        for one, k in _PAIR_SUFFIX.values():
            if name == one:
                nx[c][_PAIR_AXES[k][0]] = max(nx[c][_PAIR_AXES[k][0]], 2)
                self._pair_rows[c][k] = 2

    def _term_desc(self, loss: str, delta: float) -> "_E.MixedSystemTermDesc":
        if self._functions or self._nonlinear or self._learn:  # the parent's descriptor, with this class's pair orders
            return self._fn_desc(loss, delta)
        cv = self.coef_values
        key = (loss, float(delta))
        if key not in self._descs:
            self._descs[key] = _E.MixedSystemTermDesc(self._term_factors, self._equation_of, cv, self.dimension, self.n_fields,
                                                      self.n_equations, self._nt, self._nx, self._pair, self._eq_weights, loss, delta)
        return self._descs[key]
