"""`TermPDE`: a 1-D residual outside the nine compiled classes, given as data.

pinnrl's way to a tenth equation is a `PDEBase` subclass whose `compute_residual` combines `compute_derivatives` in
torch (pinnrl/pdes/pde_base.py:574-588).  Here the residual is a list of terms,

    r = sum_m c_m prod_f phi_{m,f},   phi in {u, u_t, u_tt, u_x, ..., u_xxxx, x, t, sin(u), cos(u)},

that `pinn_term_residual` evaluates on the jets of one `pinn_jet_forward` launch and differentiates for one
`pinn_jet_backward` launch: the residual, its loss and its gradient stay free of autograd, so everything built on the
launch list (the captured step, the flat L-BFGS closure, adaptive loss weights, the RAR sampler) takes such a PDE as it
takes the nine.  Boundary and initial conditions, samplers, loss kinds and loss weights are `PDEBase`'s.
"""

from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch

from .. import _lib
from .. import engine as _E
from .pde_base import PDEBase, PDEConfig, _jets_of, _pick_stream_set

Coef = Union[float, Tuple[float, str]]

_T_ORDER = {"u_t": 1, "u_tt": 2}
_X_ORDER = {"u_x": 1, "u_xx": 2, "u_xxx": 3, "u_xxxx": 4}


class TermPDE(PDEBase):
    """`TermPDE(config, terms, exact_solution_fn=None)` with `terms = [(coef, factors), ...]`.

    coef: a float, or `(scale, "name")` for `scale * config.parameters["name"]` (a name listed in
    `config.trainable_parameters` is a live `nn.Parameter`: such a PDE trains on the autograd step);
    factors: a tuple of the strings "u", "u_t", "u_tt", "u_x", "u_xx", "u_xxx", "u_xxxx", "x", "t", "sin(u)", "cos(u)";
    a repeated factor is a power, an empty tuple a constant source.  At most 16 terms of at most 4 factors.

    Kuramoto-Sivashinsky:  TermPDE(cfg, [(1.0, ("u_t",)), (1.0, ("u", "u_x")), (1.0, ("u_xx",)), (1.0, ("u_xxxx",))])

    The coefficient values live in one persistent device tensor (`coef_values`) that the kernel reads at launch time: an
    in-place write to it changes the PDE of every later step, a replay of a captured step included.
    """

    KIND = "term"  # not a `_lib.PDE` kind: the descriptor is a `TermDesc`

    def __init__(self, config: PDEConfig, terms: Sequence[Tuple[Coef, Sequence[str]]],
                 exact_solution_fn: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None, **kwargs):
        if int(getattr(config, "dimension", 1)) != 1:
            raise NotImplementedError(
                f"TermPDE: dimension {config.dimension}: the jet streams are pure derivatives along t and along one spatial "
                "axis, so mixed and multi-axis derivatives are not available as factors (1-D problems only)")
        terms = list(terms)
        if len(terms) > _lib.PINN_TERM_MAX_TERMS:
            raise ValueError(f"TermPDE: {len(terms)} terms; a residual has at most {_lib.PINN_TERM_MAX_TERMS}")
        self._term_coefs: List[Coef] = []
        self._term_factors: List[Tuple[str, ...]] = []
        nt = nx = 0
        for m, (coef, factors) in enumerate(terms):
            factors = (factors,) if isinstance(factors, str) else tuple(factors)
            if len(factors) > _lib.PINN_TERM_MAX_FACTORS:
                raise ValueError(f"TermPDE: term {m} has {len(factors)} factors; a term has at most {_lib.PINN_TERM_MAX_FACTORS}")
            for f in factors:
                if f not in _lib.TERM_FACTOR:
                    raise ValueError(f"TermPDE: term {m}: unknown factor '{f}' (one of {', '.join(_lib.TERM_FACTOR)})")
                nt, nx = max(nt, _T_ORDER.get(f, 0)), max(nx, _X_ORDER.get(f, 0))
            if isinstance(coef, (tuple, list)):
                if len(coef) != 2 or not isinstance(coef[1], str):
                    raise ValueError(f"TermPDE: term {m}: a coefficient is a number or (scale, 'parameter name')")
                coef = (float(coef[0]), coef[1])
            else:
                coef = float(coef)
            self._term_coefs.append(coef)
            self._term_factors.append(factors)
        try:
            self._nt, self._nx = _pick_stream_set(nt, nx)
        except NotImplementedError:
            raise NotImplementedError(
                f"TermPDE: the factors need time order {nt} together with space order {nx}, and no compiled stream set "
                "holds both (time order 2 goes with space order 0 or 2)") from None
        super().__init__(config)
        for coef in self._term_coefs:
            if isinstance(coef, tuple) and self.get_parameter(coef[1]) is None:
                raise ValueError(f"TermPDE: coefficient parameter '{coef[1]}' is not in config.parameters")
        self._exact_solution_fn = exact_solution_fn
        self._coef_values: Optional[torch.Tensor] = None
        self._coef_device: Optional[torch.device] = None
        self._descs = {}

    # ---------------------------------------------------------------- coefficients
    def _coefficients(self):
        """c_m per term: floats, or tensors where a trainable parameter enters."""
        out = []
        for coef in self._term_coefs:
            if isinstance(coef, tuple):
                p = self.get_parameter(coef[1], required=True)
                out.append(coef[0] * p)
            else:
                out.append(coef)
        return tuple(out)

    def _has_trainable_coefficients(self) -> bool:
        tr = getattr(self, "_trainable_params", {})
        return any(isinstance(c, tuple) and c[1] in tr for c in self._term_coefs)

    @property
    def coef_values(self) -> torch.Tensor:
        """The c_m as float32 on the PDE's device, one per term, built once: what the kernel reads at launch time."""
        # the REQUESTED device is remembered beside the tensor (as `_boundary_and_initial_points` does): a tensor made on
        # torch.device("cuda") reports cuda:0, which does not compare equal to the request
        dev = torch.device(self.device)
        if self._coef_values is None or self._coef_device != dev:
            vals = [float(c.detach()) if isinstance(c, torch.Tensor) else float(c) for c in self._coefficients()]
            self._coef_values = torch.tensor(vals, dtype=torch.float32, device=dev).reshape(-1)
            self._coef_device = dev
            self._descs = {}
        return self._coef_values

    def _term_desc(self, loss: str, delta: float) -> "_E.TermDesc":
        cv = self.coef_values
        key = (loss, float(delta))
        if key not in self._descs:
            self._descs[key] = _E.TermDesc(self._term_factors, cv, self._nt, self._nx, loss, delta)
        return self._descs[key]

    def _pde_desc(self):
        return self._term_desc(self._loss_function_name(), self._huber_delta())

    def _pde_desc_l1(self):
        return self._term_desc("mae", 1.0)

    # ---------------------------------------------------------------- the same formula in torch (trainable coefficients)
    def _residual_from_jets(self, j, x, nt, nx, t=None):
        u = j[0]
        val = {"u": u, "x": x.reshape(-1), "sin(u)": torch.sin(u), "cos(u)": torch.cos(u)}
        if t is not None:
            val["t"] = t.reshape(-1)
        for name, k in _T_ORDER.items():
            if k <= nt:
                val[name] = j[k]
        for name, k in _X_ORDER.items():
            if k <= nx:
                val[name] = j[nt + k]
        r = torch.zeros_like(u)
        for c, factors in zip(self._coefficients(), self._term_factors):
            term = torch.ones_like(u)
            for f in factors:
                term = term * val[f]
            r = r + c * term
        return r

    def compute_residual(self, model, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        if not self._has_trainable_coefficients():
            return super().compute_residual(model, x, t)
        jets_fn = _jets_of(model)  # a trainable coefficient stays in the graph: jets from the kernel, the formula in torch
        self._prepare_model(model)
        x = x.detach().to(self.device)
        t = t.detach().to(self.device)
        jets = jets_fn(x, t, self._nt, self._nx)
        return self._residual_from_jets(jets, x, self._nt, self._nx, t).unsqueeze(1)

    def _residual_loss(self, model, x, t, n_total=None):
        if not self._has_trainable_coefficients() or self._causal_weighting() is not None:
            # causal weighting: the base method weights the residual field of `compute_residual` above, whose torch
            # formula keeps a trainable coefficient in the graph
            return super()._residual_loss(model, x, t, n_total)
        loss = self._apply_loss_fn(self.compute_residual(model, x, t))
        if n_total is not None and int(n_total) != x.shape[0]:  # shard of a data-parallel batch: local SUM / global N
            loss = loss * (float(x.shape[0]) / float(n_total))
        return loss

    def exact_solution(self, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        if self._exact_solution_fn is None:
            raise NotImplementedError("TermPDE: no exact_solution_fn was given")
        return self._exact_solution_fn(x, t)
