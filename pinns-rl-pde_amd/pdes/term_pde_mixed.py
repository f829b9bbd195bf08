"""`TermPDEMixed`: `TermPDEnD` with mixed derivatives (u_xy, u_xxyy) and orders up to four along every space axis.

A jet launch differentiates along ONE line through input space.  `PINN_FLAG_SPACE_DIRECTION` makes that line a direction
e_a + e_b or e_a - e_b instead of an axis, and a mixed derivative is a fixed linear combination of pure derivatives along a
few such lines (polarisation).  With P_k = (d_a + d_b)^k u and Q_k = (d_a - d_b)^k u:

    u_ab   = (P_2 - u_aa - u_bb) / 2
    u_aabb = (P_4 + Q_4 - 2 u_aaaa - 2 u_bbbb) / 12

`pinn_term_residual_mixed` evaluates both inside the element-wise residual kernel and sends the cotangents back through the
transposed maps, one block per launch.  Naming "u_ab" adds the launch along e_a + e_b on the set (0, 2) and raises the orders
of the axes a and b to at least 2; naming "u_aabb" adds both direction launches on the set (0, 4) and raises the orders of
both axes to 4.  Everything else — constructor, boundary and initial handling, refusals, the launch list, the captured step,
the flat L-BFGS closure, the residual-based sampler — is `TermPDEnD`'s.

Not available: mixed space-time derivatives ("u_xt"), third-order mixed derivatives ("u_xxy", "u_xyy") and "u_xxxy"-type
factors.
"""

from __future__ import annotations

from .. import _lib
from .. import engine as _E
from .term_pde_nd import TermPDEnD


class TermPDEMixed(TermPDEnD):
    """`TermPDEMixed(config, terms, initial_condition_fn, exact_solution_fn=None)` for `config.dimension` 2 or 3.

    terms: as for `TermPDEnD`; the factor names are its names plus "u_yyy", "u_yyyy", "u_zzz", "u_zzzz", "u_xy", "u_xz",
    "u_yz", "u_xxyy", "u_xxzz", "u_yyzz" (`_lib.TERM_FACTOR_MIXED`; the z names need dimension 3).

    2-D Cahn-Hilliard, u_t = Lap(u^3 - u - eps^2 Lap u), written out:
        e2 = eps ** 2
        TermPDEMixed(cfg, [(1.0, ("u_t",)),
                           (e2, ("u_xxxx",)), (2 * e2, ("u_xxyy",)), (e2, ("u_yyyy",)),
                           (-3.0, ("u", "u", "u_xx")), (-3.0, ("u", "u", "u_yy")),
                           (-6.0, ("u", "u_x", "u_x")), (-6.0, ("u", "u_y", "u_y")),
                           (1.0, ("u_xx",)), (1.0, ("u_yy",))], initial_condition_fn)
    """

    KIND = "term_mixed"  # not a `_lib.PDE` kind: the descriptor is a `MixedTermDesc`
    _FACTORS = _lib.TERM_FACTOR_MIXED
    _AXIS_ORDER = dict(TermPDEnD._AXIS_ORDER, u_yyy=(1, 3), u_yyyy=(1, 4), u_zzz=(2, 3), u_zzzz=(2, 4))
    _PAIR_ORDER = {"u_xy": (0, 2), "u_xz": (1, 2), "u_yz": (2, 2), "u_xxyy": (0, 4), "u_xxzz": (1, 4), "u_yyzz": (2, 4)}
    _FACTOR_NOTE = ("mixed space-time derivatives (u_xt), third-order mixed derivatives (u_xxy, u_xyy) and u_xxxy-type factors "
                    "are not available")

    def _term_desc(self, loss: str, delta: float) -> "_E.MixedTermDesc":
        cv = self.coef_values
        key = (loss, float(delta))
        if key not in self._descs:
            self._descs[key] = _E.MixedTermDesc(self._term_factors, cv, self.dimension, self._nt, self._nx, self._pair, loss, delta)
        return self._descs[key]
