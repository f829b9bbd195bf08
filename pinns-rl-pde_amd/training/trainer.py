"""`PDETrainer` — counterpart of pinnrl/training/trainer.py for the accelerated path.

The step semantics of the reference's inner loop (trainer.py:539-698) are reproduced exactly:
`steps/epoch = num_points // batch_size`; fresh sample each step (strategy "adaptive" when an RL
agent is attached, else `config.training.collocation_distribution`); `zero_grad -> compute_loss ->
[adaptive weights] -> backward -> clip_grad_norm_ -> optimizer.step`; per-epoch scheduler step;
validation every `validation_frequency` epochs on 1000 (-> 961) points; early stopping on
`val < best - 1e-6`.  Like upstream, `optimizer_config` is accepted and ignored (lr / weight decay
come from `config.training`, trainer.py:292-297).  Plotting, JSON metadata, live snapshots and the
tqdm bar are dashboard plumbing and out of scope; `loss.item()` host syncs happen once per epoch
(plus `log_every_step=True` for reference-identical per-step bookkeeping).

Data-parallel (new): pass `process_group=` (one process per GPU).  Each rank trains
on its shard of every batch; ONE all-reduce per step carries [flat gradient || loss terms].
"""

from __future__ import annotations

import logging
from datetime import datetime
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from .. import distributed as _D
from .. import engine as _E
from .._lib import LBFGS_REC, PINN_ADAPTIVE_SCRATCH_FLOATS, PINN_CAUSAL_SCRATCH_DOUBLES, PINN_FACE_SCRATCH_DOUBLES, PINN_FD_SCRATCH_DOUBLES, PINN_LBFGS_MAX_HISTORY, PINN_LBFGS_RECORD_DOUBLES
from ..config import validate_causal_eps
from .lbfgs import LBFGSDriver


class _EmaLossWeights:
    """The two EMA rules of pinnrl/components/adaptive_weights.py:31-111 (scalar bookkeeping on 3-4 numbers)."""

    def __init__(self, strategy="rbw", alpha=0.9, eps=1e-5, initial_weights=None):
        self.strategy, self.alpha, self.eps = strategy.lower(), alpha, float(eps)
        self.initial_weights = torch.tensor(initial_weights) if initial_weights is not None else None
        self.weights = self.running = self.prev_weights = None

    def update(self, losses=None, gradients=None):
        v = gradients if (self.strategy == "lrw" and gradients is not None) else losses
        if v is None or (self.strategy not in ("lrw", "rbw")):
            raise ValueError(f"Invalid combination of strategy ({self.strategy}) and inputs")
        if self.running is None:
            self.running = v
            self.weights = self.initial_weights.to(v.device) if self.initial_weights is not None else torch.ones_like(v)
            return self.weights
        self.running = self.alpha * self.running + (1 - self.alpha) * v
        if self.strategy == "lrw":
            inv = 1.0 / (self.running + self.eps)
            self.weights = inv / torch.sum(inv)
        else:
            self.weights = self.running / (self.running.sum() + self.eps)
            if self.prev_weights is not None:
                self.weights = self.alpha * self.prev_weights + (1 - self.alpha) * self.weights
            self.prev_weights = self.weights.clone()
        return self.weights


class _FlatLBFGSBackend:
    """What `LBFGSDriver` asks for, as launches over the flat buffers of a `PDETrainer`.  `evaluate` and `direction` block
    once each, on the copy of the 72-double record into pinned host memory; nothing else is read on the host."""

    def __init__(self, trainer, L):
        self.tr, self.L = trainer, L

    def _read(self):
        L = self.L
        L["host"].copy_(L["record"], non_blocking=True)
        torch.cuda.current_stream(self.tr.device).synchronize()
        return L["host"].tolist()

    def reset(self):
        self.L["state"].zero_()
        self.L["d"].zero_()

    def evaluate(self, t):
        tr, L = self.tr, self.L
        F = tr._flat
        if t is not None:
            torch.add(L["x0"], L["d"], alpha=float(t), out=F["theta"])
        x, tt = L["batch"]
        tr._loss_grad_launches(x, tt, F, tr.model.program(), tr.pde._pde_desc(), tr._chain(x.shape[0]))
        _E.lbfgs_eval_stats(F["grad"], L["d"], F["summary"][3:4], L["scratch"], L["record"])
        rec = self._read()
        return {k: rec[LBFGS_REC[k]] for k in ("loss", "gtd", "gmax", "gsum")}

    def direction(self, t_prev):
        L = self.L
        _E.lbfgs_direction(self.tr._flat["grad"], L["prev_grad"], L["d"], L["ring"], L["history_size"], float(t_prev),
                           L["state"], L["scratch"], L["record"])
        return _E.lbfgs_record(self._read())

    def snapshot(self):
        self.L["x0"].copy_(self.tr._flat["theta"])

    def accept(self, t):
        torch.add(self.L["x0"], self.L["d"], alpha=float(t), out=self.tr._flat["theta"])

    def save(self, slot):
        self.L["slots"][slot].copy_(self.tr._flat["grad"][: self.L["n"]])

    def restore(self, slot):
        self.tr._flat["grad"][: self.L["n"]].copy_(self.L["slots"][slot])


class PDETrainer:
    def __init__(self, model: nn.Module, pde, optimizer_config: Optional[Dict], config, device: Optional[torch.device] = None,
                 rl_agent=None, viz_frequency=10, validation_frequency=10, early_stopping_config=None,
                 process_group=None, log_every_step: bool = False, fast_step: Optional[bool] = None):
        self.device = device or (config.device if hasattr(config, "device") else torch.device("cpu"))
        self.model = model.to(self.device)
        self.pde = pde
        self.config = config
        self.validation_frequency = validation_frequency
        self.logger = logging.getLogger(__name__)
        self.process_group = process_group
        self.log_every_step = log_every_step
        # fast_step: None = `train()` takes the autograd-free launch list whenever it covers the configuration
        # (`_manual_step_unsupported()` is None) and the device is a GPU; False = always the autograd step; True = require it
        self.fast_step = fast_step
        if self._causal is not None:
            if process_group is not None:
                raise NotImplementedError("causal weighting under a process group: the bin means would need their own collective")
            if getattr(config.training, "optimizer", "adam") != "adam":
                raise NotImplementedError("causal weighting with L-BFGS: the weights are detached, so the function the line "
                                          "search sees is not the one the gradient belongs to")
            t_lo, t_hi = float(self.pde.time_domain[0]), float(self.pde.time_domain[1])
            if not (np.isfinite(t_lo) and np.isfinite(t_hi) and t_hi > t_lo):
                raise ValueError(f"causal weighting needs a finite time domain with t_hi > t_lo, got ({t_lo}, {t_hi})")
        if process_group is not None:
            # replicas must start from ONE theta_0 and apply identical updates: broadcast rank 0's parameters,
            # and refuse the modes whose per-rank quantities this path does not reduce
            if config.training.adaptive_weights.enabled:
                raise NotImplementedError("data-parallel training supports fixed loss weights only: the EMA weight rules "
                                          "need every loss component reduced over ranks before the update")
            _D.broadcast_parameters(self.model, process_group)
            if hasattr(self.pde, "_trainable_params") and len(self.pde._trainable_params):
                _D.broadcast_parameters(self.pde._trainable_params, process_group)
        self._initialize_optimizer_and_scheduler()
        self.history = {"train_loss": [], "val_loss": [], "residual_loss": [], "boundary_loss": [], "initial_loss": [],
                        "learning_rate": [], "loss_weights": []}
        if early_stopping_config is None:
            early_stopping_config = {"enabled": True, "patience": 10}
        self.early_stopping_enabled = early_stopping_config.get("enabled", True)
        self.patience = early_stopping_config.get("patience", 10)
        self.best_val_loss = float("inf")
        self.patience_counter = 0
        self.rl_agent = rl_agent
        self.viz_frequency = viz_frequency
        aw = config.training.adaptive_weights
        self.use_adaptive_weights = bool(aw.enabled)
        self.adaptive_weights = (
            _EmaLossWeights(aw.strategy, aw.alpha, aw.eps, aw.initial_weights) if self.use_adaptive_weights else None
        )
        self._pending_weights: List[torch.Tensor] = []  # device copies of the launch-list steps' weights, see `_flush_loss_weights`
        self.points_history: List[np.ndarray] = []

    @property
    def _causal(self):
        """(num_bins, eps) of the causal weighting, or None when it is off — read from the PDE's training config on every
        use, the one place the autograd path (`PDEBase._residual_loss`) reads it from too."""
        return self.pde._causal_weighting() if hasattr(self.pde, "_causal_weighting") else None

    def _sync_causal_state(self, F, causal):
        """Bring the launch list's device-side sharpness in step with the config before an eager step.  The bin count sizes
        persistent buffers, so it is fixed once the flat state exists.  Not during graph capture: a captured fill would
        reset the sharpness on every replay; a captured step follows `set_causal_eps` alone."""
        built = F.get("causal_host")
        if built is None or built[0] != causal[0]:
            raise RuntimeError("causal_weighting was enabled, or its num_bins changed, after the trainer's flat state was built: "
                               "build a new PDETrainer")
        if built[1] != causal[1] and not (F["causal_eps"].is_cuda and torch.cuda.is_current_stream_capturing()):
            F["causal_eps"].fill_(causal[1])
            F["causal_host"] = causal

    # ---------------------------------------------------------------- optimizer / scheduler (trainer.py:281-371)
    def _collect_optimizable_params(self):
        params = list(self.model.parameters())
        if hasattr(self.pde, "trainable_parameters_iter"):
            params += list(self.pde.trainable_parameters_iter())
        return params

    def _build_adam(self, params):
        tc = self.config.training
        # same update rule as the reference's optim.Adam(lr, weight_decay) (trainer.py:292-297); on the device the
        # multi-tensor update runs as ONE fused kernel instead of ~10 foreach launches
        fused = all(p.is_cuda and p.dtype == torch.float32 for p in params)
        return optim.Adam(params, lr=tc.learning_rate, weight_decay=tc.weight_decay, fused=fused)

    def _build_lbfgs(self, params):
        tc, c = self.config.training, self.config.training.lbfgs
        return optim.LBFGS(params, lr=tc.learning_rate, history_size=c.history_size, max_iter=c.max_iter,
                           line_search_fn=c.line_search_fn, tolerance_grad=c.tolerance_grad,
                           tolerance_change=c.tolerance_change)

    def _build_scheduler(self, force_reduce_lr: bool = False):
        sc = self.config.training.learning_rate_scheduler
        if force_reduce_lr or sc.type == "reduce_lr":
            return optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, mode="min", factor=sc.factor,
                                                        patience=sc.patience, min_lr=sc.min_lr)
        if sc.type == "cosine":
            return optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=self.config.training.num_epochs,
                                                        eta_min=sc.min_lr)
        raise ValueError(f"Unknown scheduler type: {sc.type}")

    def _initialize_optimizer_and_scheduler(self):
        kind = getattr(self.config.training, "optimizer", "adam")
        params = self._collect_optimizable_params()
        self._is_lbfgs = kind == "lbfgs"
        self.optimizer = self._build_lbfgs(params) if self._is_lbfgs else self._build_adam(params)
        if kind == "adam_lbfgs":
            ratio = getattr(self.config.training, "adam_lbfgs_switch_ratio", 0.7)
            self._switch_epoch = max(1, int(self.config.training.num_epochs * ratio))
        else:
            self._switch_epoch = None
        self.scheduler = self._build_scheduler(force_reduce_lr=self._is_lbfgs)
        self._optimizer_type = kind

    def _switch_to_lbfgs(self):
        """The hand-over of `adam_lbfgs` (trainer.py:339-371): a fresh torch.optim.LBFGS and a ReduceLROnPlateau scheduler.
        On a flat state (the Adam phase ran the launch list) the step form switches to `_lbfgs_step_flat` and starts from an
        empty history, like the fresh optimiser; the torch objects stay, for `param_groups["lr"]`."""
        self.optimizer = self._build_lbfgs(self._collect_optimizable_params())
        self._is_lbfgs = True
        self.scheduler = self._build_scheduler(force_reduce_lr=True)
        if getattr(self, "_flat", None) is not None:
            self.optimizer._opt_called = True  # the flat L-BFGS steps; the scheduler only reads / writes param_groups
            if "lbfgs" in self._flat:
                self._flat["lbfgs"]["driver"].reset()

    def _update_scheduler(self, val_loss=None):
        if isinstance(self.scheduler, optim.lr_scheduler.ReduceLROnPlateau):
            self.scheduler.step(val_loss)
        else:
            self.scheduler.step()

    # ---------------------------------------------------------------- validation (trainer.py:140-162)
    def _compute_validation_loss(self, num_points: int = 1000) -> Dict[str, float]:
        self.model.eval()
        x, t = self.pde.generate_collocation_points(num_points)
        with torch.no_grad():  # forward-only fused kernels; the reference builds (and discards) a graph here
            losses = self.pde.compute_loss(self.model, x.to(self.device), t.to(self.device))
        vals = torch.stack([losses[k].detach().reshape(()).float() for k in ("total", "residual", "boundary", "initial")])
        if self.process_group is not None:  # rank-local random validation points: average, so every rank stops together
            torch.distributed.all_reduce(vals, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
            vals = vals / torch.distributed.get_world_size(self.process_group)
        v = vals.tolist()
        return {"total_loss": v[0], "residual_loss": v[1], "boundary_loss": v[2], "initial_loss": v[3]}

    # ---------------------------------------------------------------- live snapshot (trainer.py:171-279)
    def live_snapshot_fields(self, grid_size: int = 60) -> Dict[str, object]:
        """The fields of the reference's `_save_live_snapshot` — predicted u and the PDE residual on a fixed
        grid_size x grid_size grid (x-t in 1-D; x1-x2 at the mid time in >= 2-D) — from two forward-only launches (no
        autograd graph; the reference builds one for the residual and throws it away).  Same keys as its `.npz`."""
        dev = self.device
        dim = int(getattr(self.pde, "dimension", 1))
        t_lo, t_hi = float(self.pde.time_domain[0]), float(self.pde.time_domain[1])
        if dim <= 1:
            xs = np.linspace(float(self.pde.domain[0][0]), float(self.pde.domain[0][1]), grid_size, dtype=np.float32)
            ys = np.linspace(t_lo, t_hi, grid_size, dtype=np.float32)
            xx, tt = np.meshgrid(xs, ys, indexing="xy")
            x_flat = torch.tensor(xx.reshape(-1, 1), device=dev)
            t_flat = torch.tensor(tt.reshape(-1, 1), device=dev)
            meta = {"dimension": 1, "x_label": "x", "y_label": "t", "fixed_t": float("nan")}
        else:
            xs = np.linspace(float(self.pde.domain[0][0]), float(self.pde.domain[0][1]), grid_size, dtype=np.float32)
            ys = np.linspace(float(self.pde.domain[1][0]), float(self.pde.domain[1][1]), grid_size, dtype=np.float32)
            xx1, xx2 = np.meshgrid(xs, ys, indexing="xy")
            cols = [xx1.reshape(-1), xx2.reshape(-1)] + [np.full(xx1.size, 0.5 * (float(self.pde.domain[d][0]) + float(self.pde.domain[d][1])),
                                                                 dtype=np.float32) for d in range(2, dim)]
            x_flat = torch.tensor(np.stack(cols, axis=1), device=dev, dtype=torch.float32)
            fixed_t = 0.5 * (t_lo + t_hi)
            t_flat = torch.full((x_flat.shape[0], 1), fixed_t, dtype=torch.float32, device=dev)
            meta = {"dimension": 2, "x_label": "x1", "y_label": "x2", "fixed_t": float(fixed_t)}
        was_training = self.model.training
        try:
            with torch.no_grad():
                u = self.model(torch.cat([x_flat, t_flat], dim=1))
                r = self.pde.compute_residual(self.model, x_flat, t_flat)  # forward-only kernel under no_grad
        finally:
            self.model.train(was_training)
        out = {"axis_x": xs, "axis_y": ys, "u_pred": u.detach().cpu().numpy()[:, 0].reshape(grid_size, grid_size),
               "residual": r.detach().cpu().numpy().reshape(grid_size, grid_size)}
        out.update(meta)
        return out

    def _save_live_snapshot(self, experiment_dir: str, epoch: int, grid_size: int = 60) -> None:
        if not experiment_dir:
            return
        try:
            import os

            np.savez(os.path.join(experiment_dir, "live_snapshot.npz"), epoch=int(epoch), **self.live_snapshot_fields(grid_size))
        except Exception as exc:  # viz must never crash the training loop (trainer.py:186-188)
            self.logger.debug(f"Live snapshot skipped: {exc}")

    # ---------------------------------------------------------------- one step
    def _sample(self, batch_size: int):
        strategy = "adaptive" if self.rl_agent is not None else self.config.training.collocation_distribution
        if strategy == "adaptive" and getattr(self, "_flat", None) is not None and hasattr(self.pde, "_sample_adaptive_device"):
            # the autograd-free step samples without a host round trip (device-side action selection and epsilon decay)
            if getattr(self.pde, "rl_agent", None) is None:
                self.pde.rl_agent = self.rl_agent
            return self.pde._sample_adaptive_device(batch_size)
        kw = {"model": self.model} if strategy == "residual_based" else {}
        x, t = self.pde.generate_collocation_points(batch_size, strategy=strategy, **kw)
        return x.to(self.device), t.to(self.device)

    def _lbfgs_step(self, x, t):  # trainer.py:373-389
        captured: Dict[str, Dict] = {}

        def closure():
            self.optimizer.zero_grad()
            losses = self._losses(x, t)
            losses["total"].backward()
            self._sync_grads(losses)
            captured["losses"] = losses
            return losses["total"]

        self.optimizer.step(closure)
        if "losses" not in captured:
            captured["losses"] = self._losses(x, t)
        return captured["losses"]

    def _lbfgs_flat_state(self):
        """The flat L-BFGS beside the flat parameters: ring, prev_grad, direction and the double block of
        `pinn_lbfgs_direction`, x0 and three rotating gradient buffers for the line search, a pinned host copy of the
        record, and the `LBFGSDriver` whose backend these launches are."""
        F = self._flat
        L = F.get("lbfgs")
        if L is None:
            c = self.config.training.lbfgs
            n, dev = F["n"], self.device
            L = _E.lbfgs_buffers(n, int(c.history_size), dev)
            L["x0"] = torch.zeros(n, dtype=torch.float32, device=dev)
            L["slots"] = torch.zeros(3, n, dtype=torch.float32, device=dev)
            L["host"] = torch.zeros(PINN_LBFGS_RECORD_DOUBLES, dtype=torch.float64).pin_memory()
            L["batch"] = None
            L["driver"] = LBFGSDriver(_FlatLBFGSBackend(self, L), max_iter=c.max_iter, tolerance_grad=c.tolerance_grad,
                                      tolerance_change=c.tolerance_change, line_search_fn=c.line_search_fn,
                                      lr=lambda: self.optimizer.param_groups[0]["lr"])
            F["lbfgs"] = L
        return L

    def _lbfgs_step_flat(self, x, t):
        """`optimizer.step(closure)` of torch.optim.LBFGS on the flat buffers: every closure evaluation is the launch list
        without its optimiser tail plus `pinn_lbfgs_eval_stats`, every iteration one `pinn_lbfgs_direction`; the host
        decides on the records (`LBFGSDriver`).  Returns the summary of the LAST evaluation, as the eager closure does."""
        L = self._lbfgs_flat_state()
        L["batch"] = (x, t)
        try:
            L["driver"].step()
        finally:
            L["batch"] = None
        return self._manual_losses()

    def _losses(self, x, t):
        if self.process_group is not None:
            return _D.sharded_compute_loss(self.pde, self.model, x, t, self.process_group)
        return self.pde.compute_loss(self.model, x, t)

    def _ensure_dp_buffer(self):
        """Every parameter's `.grad` becomes a VIEW of one persistent [gradients || 4 scalars] buffer: backward
        accumulates straight into it and the step's single all-reduce runs on it in place (no cat / copy-back)."""
        if getattr(self, "_dp_buf", None) is not None:
            return
        params = self._collect_optimizable_params()
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        buf = torch.zeros(n + 4, dtype=torch.float32, device=params[0].device)
        for p, o in zip(params, offs):
            p.grad = buf[o : o + p.numel()].view_as(p)
        self._dp_buf, self._dp_n = buf, n

    def _sync_grads(self, losses=None):
        """ONE all-reduce of [gradients || residual loss]; the reduced (global) residual replaces the local shard's."""
        if self.process_group is None:
            return
        red = None
        if getattr(self, "_dp_buf", None) is not None:
            buf = self._dp_buf
            if losses is not None:
                buf[self._dp_n] = losses["residual"].detach().reshape(())
            torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
            red = buf[self._dp_n : self._dp_n + 1]
        else:
            scalars = [losses["residual"]] if losses is not None else None
            red = _D.all_reduce_gradients(self._collect_optimizable_params(), self.process_group, scalars=scalars)
        if red is not None and losses is not None:
            world = torch.distributed.get_world_size(self.process_group)
            local = losses["residual"].detach()
            losses["residual"] = red[0].clone()
            # local total = rw * local_residual + (aux terms) / world  ->  global total (for logging only)
            lw = self.pde._loss_weights() if hasattr(self.pde, "_loss_weights") else None
            rw = (lw.get("pde", lw.get("residual", 1.0)) if lw else 1.0)
            losses["total"] = (losses["total"].detach() - rw * local) * world + rw * red[0]

    def _adaptive_total(self, losses):
        """trainer.py:586-684 without the printing: reweight residual/boundary/initial (+ smoothness)."""
        tc = self.config.training
        names = ["residual", "boundary", "initial"]
        if "smoothness" in losses and tc.loss_weights.get("smoothness", 0.0) > 0:
            names.append("smoothness")
        comps = torch.stack([losses[n].detach().reshape(()) for n in names])
        if tc.adaptive_weights.strategy == "lrw":
            norms = []
            for n in names:
                self.optimizer.zero_grad()
                losses[n].backward(retain_graph=True)
                sq = sum(float(p.grad.norm().item()) ** 2 for p in self.model.parameters() if p.grad is not None)
                norms.append(torch.tensor(sq**0.5, device=self.device))
            self.optimizer.zero_grad()
            weights = self.adaptive_weights.update(gradients=torch.stack(norms))
        else:
            weights = self.adaptive_weights.update(losses=comps)
        total = 0
        for i, n in enumerate(names):
            if i < len(weights):
                total = total + weights[i] * losses[n]
        if tc.mode in ("inverse", "data_augmented") and "data" in losses:
            total = total + (tc.loss_weights.get("data", 1.0) or 1.0) * losses["data"]
        w = weights.detach().cpu().numpy()
        if len(w) < 4:
            w = np.concatenate([w, np.zeros(4 - len(w))])
        self.history["loss_weights"].append(w)
        return total

    def train_step(self, x, t):
        """zero_grad -> compute_loss -> backward -> clip -> step  (trainer.py:576-694)."""
        if self._is_lbfgs:
            if getattr(self, "_flat", None) is not None:
                return self._lbfgs_step_flat(x, t)
            return self._lbfgs_step(x, t)
        if getattr(self, "_flat", None) is not None:  # parameters live in the flat buffers: same sequence, not captured
            self._manual_launches(x, t)
            losses = self._manual_losses()
            if "weights" in losses:  # one `history["loss_weights"]` row per step, as `_adaptive_total` appends them
                self._pending_weights.append(losses["weights"])
            return losses
        if self.process_group is not None:
            self._ensure_dp_buffer()
            self._dp_buf.zero_()  # the .grad views stay attached (zero_grad(set_to_none=True) would drop them)
        else:
            self.optimizer.zero_grad()
        losses = self._losses(x, t)
        if self.use_adaptive_weights and self.config.training.mode != "data_only":
            losses["total"] = self._adaptive_total(losses)
        losses["total"].backward()
        self._sync_grads(losses)
        gc = self.config.training.gradient_clipping
        if gc > 0:
            nn.utils.clip_grad_norm_(self.model.parameters(), gc)
        self.optimizer.step()
        return losses

    # ---------------------------------------------------------------- autograd-free step
    def _manual_step_unsupported(self) -> Optional[str]:
        """None when the step can run as the fixed launch sequence below; else the reason (callers fall back)."""
        from ..pdes.pde_base import PDEBase
        from ..pdes.term_pde import TermPDE
        from ..pdes.term_pde_nd import TermPDEnD
        from ..pdes.term_pde_system import TermPDESystem

        tc = self.config.training
        kind = getattr(tc, "optimizer", "adam")
        if kind not in ("adam", "lbfgs", "adam_lbfgs") or (self._is_lbfgs and kind == "adam"):
            return "optimizer is not Adam or L-BFGS"
        if kind != "adam":
            why = self._lbfgs_step_unsupported()
            if why is not None:
                return why
        nd = isinstance(self.pde, TermPDEnD)
        if nd:
            # a term residual in 2 or 3 space dimensions: the chain of `engine.residual_loss_grad` over the axes and the class's
            # own boundary / initial chain cover Adam with fixed loss weights and L-BFGS on one device
            if self.use_adaptive_weights:
                return "TermPDEnD with adaptive loss weights"
            if self._causal is not None:
                return "TermPDEnD with causal weighting"
            if self.process_group is not None:
                return "TermPDEnD under a process group"
            if self.rl_agent is not None:
                return "TermPDEnD with an RL agent (the agent's grid sampler is the 1-D launch list's)"
        system = isinstance(self.pde, TermPDESystem)
        if system:
            # a coupled system: the chain of `engine.residual_loss_grad` over the fields and their axes (component launches) and
            # the class's own boundary / initial chain cover Adam with fixed loss weights and L-BFGS on one device, with the
            # uniform and the stratified sampler
            if self.use_adaptive_weights:
                return "TermPDESystem with adaptive loss weights (the three components would be sums over fields and equations)"
            if self._causal is not None:
                return "TermPDESystem with causal weighting (pinn_causal_weights takes one residual field)"
            if self.process_group is not None:
                return "TermPDESystem under a process group"
            if self.rl_agent is not None:
                return "TermPDESystem with an RL agent (the agent's reward is one residual field)"
            if getattr(tc, "collocation_distribution", "uniform") == "residual_based":
                return "TermPDESystem with the residual-based sampler (its weights come from one residual field)"
            if len(getattr(self.pde, "_trainable_params", {})):
                return "TermPDESystem with trainable parameters (the coefficients of a term residual are read by value)"
            if self.pde._training_mode() != "forward" or getattr(self.pde, "observation_data", None):
                return "TermPDESystem in a data mode (the launch list of a system covers forward problems)"
            n_out = getattr(getattr(self.model, "model", self.model), "output_dim", None)
            if n_out != self.pde.n_fields:
                return f"TermPDESystem with {self.pde.n_fields} fields on a model whose output_dim is {n_out}"
        if self.rl_agent is not None and not hasattr(self.rl_agent, "action_probabilities"):
            return "RL agent without a device-side action selection"
        if getattr(tc, "collocation_distribution", "uniform") not in ("uniform", "stratified", "residual_based"):
            return "unknown sampler"
        if self._causal is not None:
            # causal weighting: the residual launch becomes forward -> pinn_causal_weights -> reverse; that chain covers a
            # forward problem with fixed loss weights and coefficients by value
            if self.use_adaptive_weights:
                return "causal weighting with adaptive loss weights"
            if len(getattr(self.pde, "_trainable_params", {})) or self.pde._has_trainable_coefficients():
                return "causal weighting with trainable PDE coefficients"
            if self.pde._training_mode() != "forward" or getattr(self.pde, "observation_data", None):
                return "causal weighting with a data mode or an observation-data term"
            if (self.pde._loss_weights() or {}).get("smoothness", 0.0) > 0 and type(self.pde).compute_loss is not PDEBase.compute_loss:
                return "causal weighting with a smoothness term"
        if isinstance(self.pde, TermPDE):
            # a residual given as data runs the launch list through the chain jets -> pinn_term_residual -> reverse sweep
            # (engine.residual_loss_grad dispatches on the descriptor), with its coefficients by value on the device
            if self.pde._has_trainable_coefficients():  # a trainable parameter no term names gets the general reason below
                return ("TermPDE with trainable term coefficients (the flat coefficient state of the inverse launch list has "
                        "two slots, a term residual up to sixteen coefficients)")
            if self.pde._training_mode() != "forward" or getattr(self.pde, "observation_data", None):
                return "TermPDE in a data mode (the launch list of a term residual covers forward problems)"
            if self.process_group is not None:
                return "TermPDE under a process group"
        own_loss = type(self.pde).compute_loss is not PDEBase.compute_loss
        if own_loss and type(self.pde)._manual_chain is PDEBase._manual_chain:
            return f"{type(self.pde).__name__} overrides compute_loss without a launch-list form (_manual_chain)"
        if own_loss and (self.pde._loss_weights() or {}).get("smoothness", 0.0) > 0:
            if self.pde._manual_smoothness() is None:
                return "smoothness term"
            if self.process_group is not None:
                return "smoothness term under a process group"
        if self.pde.dimension != 1 and not nd and not system:
            return "multi-dimensional problem"
        mode = self.pde._training_mode()
        if mode == "data_only":
            return "data_only mode"
        if mode not in ("forward", "inverse", "data_augmented"):
            return f"unknown training mode '{mode}'"
        inverse = bool(len(getattr(self.pde, "_trainable_params", {}))) or self.pde._has_trainable_coefficients()
        if inverse:
            if self._coefficient_slots() is None:
                return ("trainable parameters that are not themselves kernel coefficients (the residual reads a function "
                        "of them: needs a chain rule)")
            if self.rl_agent is not None or getattr(tc, "collocation_distribution", "uniform") == "residual_based":
                return "residual-based or RL sampling with trainable coefficients (the sampler's launch takes coefficients by value)"
        if self.process_group is not None and (inverse or mode != "forward"):
            return "inverse or data-driven mode under a process group"
        if getattr(self.pde, "observation_data", None) and mode == "forward":
            return "observation data term"
        ic = getattr(self.pde.config, "initial_condition", None) or {}
        if ic.get("type") == "random":
            return "random initial condition"
        if self.use_adaptive_weights:
            return self._adaptive_step_unsupported(mode, inverse)
        return None

    def _lbfgs_step_unsupported(self) -> Optional[str]:
        """What keeps an `lbfgs` / `adam_lbfgs` run on the eager `_lbfgs_step` (and the Adam phase before it on the autograd
        step): the flat L-BFGS state covers the network's parameters alone, on one device, with fixed loss weights."""
        tc = self.config.training
        if len(getattr(self.pde, "_trainable_params", {})) or self.pde._has_trainable_coefficients():
            return "L-BFGS with trainable PDE coefficients (the flat vector would be [theta || coefficients])"
        if getattr(self.pde, "_learn", ()):
            return "L-BFGS with learn (learnable parameters of a term system: the flat vector would be [theta || parameters])"
        if self.process_group is not None:
            return "L-BFGS under a process group"
        if self.use_adaptive_weights:
            return "L-BFGS with adaptive loss weights"
        if int(tc.lbfgs.history_size) > PINN_LBFGS_MAX_HISTORY:
            return f"L-BFGS history_size {int(tc.lbfgs.history_size)} > {PINN_LBFGS_MAX_HISTORY}"
        if int(tc.lbfgs.history_size) < 1:
            return "L-BFGS history_size < 1"
        return None

    def _adaptive_step_unsupported(self, mode: str, inverse: bool) -> Optional[str]:
        """What keeps adaptive loss weights (RBW / LRW) on the eager step: the launch list reweights exactly the three
        components residual / boundary / initial of a forward problem."""
        tc = self.config.training
        aw = tc.adaptive_weights
        if aw.strategy not in ("rbw", "lrw"):  # as `_adaptive_total` spells them; any other spelling keeps its eager behaviour
            return f"adaptive loss weights with strategy '{aw.strategy}'"
        if mode != "forward" or getattr(tc, "mode", "forward") != "forward":
            return "adaptive loss weights outside forward mode (the data term is added unweighted after the reweighting)"
        if inverse:
            return "adaptive loss weights with trainable PDE coefficients"
        if getattr(self.pde, "observation_data", None):
            return "adaptive loss weights with an observation-data term"
        if (getattr(tc, "loss_weights", None) or {}).get("smoothness", 0.0) > 0:
            return "adaptive loss weights with a smoothness component"
        if aw.initial_weights is not None and len(aw.initial_weights) != 3:
            return f"adaptive loss weights with {len(aw.initial_weights)} initial weights (the step has three components)"
        if self.process_group is not None:
            return "adaptive loss weights under a process group"
        return None

    def _coefficient_slots(self):
        """{slot k of `pde._coefficients()`: its nn.Parameter} when every trainable parameter of the PDE IS one of the (at
        most two differentiated) kernel coefficients; None when some trainable parameter reaches the residual through a
        function (pendulum's c0 = g / L) or not at all."""
        params = list(getattr(self.pde, "_trainable_params", {}).values())
        coefs = list(self.pde._coefficients())
        slots = {}
        for k, c in enumerate(coefs):
            if isinstance(c, torch.Tensor) and c.requires_grad:
                hit = [p for p in params if p is c]
                if not hit or k >= 2 or c.numel() != 1:
                    return None
                slots[k] = hit[0]
        if len(slots) != len(params):
            return None
        return slots

    def _build_flat_state(self):
        """Move the parameters into ONE flat fp32 buffer (each `nn.Parameter` becomes a view of it, same layout as the
        engine's flat gradient) with flat Adam moments beside it; Adam state of eager steps taken so far comes along.
        The history of eager L-BFGS steps taken before the flat state exists does NOT come along: the flat L-BFGS starts
        from an empty history (torch keeps its pairs per parameter list; `train()` builds the flat state before its first
        step, so this only concerns `train_step` calls made before it)."""
        if getattr(self, "_flat", None) is not None:
            return self._flat
        prog = self.model.program()
        offs, n = prog.grad_layout()
        dev = self.device
        theta = torch.zeros(n, dtype=torch.float32, device=dev)
        m, v = torch.zeros_like(theta), torch.zeros_like(theta)
        steps = 0.0
        with torch.no_grad():
            for p, o in zip(prog.tensors, offs):
                if o < 0:
                    continue
                view = theta[o : o + p.numel()].view_as(p)
                view.copy_(p.data)
                st = self.optimizer.state.get(p, {})
                if "exp_avg" in st:
                    m[o : o + p.numel()].view_as(p).copy_(st["exp_avg"])
                    v[o : o + p.numel()].view_as(p).copy_(st["exp_avg_sq"])
                    steps = float(st["step"])
                p.data = view
        g = self.optimizer.param_groups[0]
        self.optimizer._opt_called = True  # the flat Adam kernel steps from now on; schedulers only read / write param_groups
        lw = self.pde._loss_weights()
        rw = lw.get("pde", lw.get("residual", 1.0)) if lw else 1.0
        self._flat = {
            "theta": theta, "m": m, "v": v, "grad": torch.zeros(n + 4, dtype=torch.float32, device=dev),
            "step": torch.tensor([steps], dtype=torch.float32, device=dev),
            "lr": torch.tensor([g["lr"]], dtype=torch.float32, device=dev),
            "scratch": torch.zeros(64, dtype=torch.float32, device=dev), "n": n, "rw": float(rw), "chains": {},
            "grad_side": torch.zeros(n, dtype=torch.float32, device=dev),
            "summary": torch.zeros(4, dtype=torch.float32, device=dev),
            "betas": g.get("betas", (0.9, 0.999)), "eps": g.get("eps", 1e-8), "wd": g.get("weight_decay", 0.0),
        }
        slots = self._coefficient_slots() if len(getattr(self.pde, "_trainable_params", {})) else None
        if slots:
            # inverse problems: the PDE coefficients live in a 4-float device buffer in `_coefficients()` order (what
            # pinn_residual_loss_grad_inverse reads at launch time); each trainable nn.Parameter becomes a view of its slot,
            # with its own Adam moments and step counter.  Non-trainable entries hold their constants.
            F = self._flat
            coef = torch.zeros(4, dtype=torch.float32, device=dev)
            cm, cv = torch.zeros_like(coef), torch.zeros_like(coef)
            csteps = 0.0
            with torch.no_grad():
                for k, c in enumerate(self.pde._coefficients()):
                    if k in slots:
                        p = slots[k]
                        coef[k : k + 1].copy_(p.data.reshape(1))
                        st = self.optimizer.state.get(p, {})
                        if "exp_avg" in st:
                            cm[k : k + 1].copy_(st["exp_avg"].reshape(1))
                            cv[k : k + 1].copy_(st["exp_avg_sq"].reshape(1))
                            csteps = float(st["step"])
                        p.data = coef[k]
                    else:
                        coef[k] = float(c)
            lo, hi = min(slots), max(slots) + 1  # at most two coefficients: the trainable ones are a contiguous slice
            F["grad"] = torch.zeros(n + 8, dtype=torch.float32, device=dev)  # [gradient | loss sum, pad | coefficient gradients]
            F.update({"coef": coef, "coef_m": cm, "coef_v": cv, "coef_grad": F["grad"][n + 4 : n + 8], "coef_slice": (lo, hi),
                      "coef_step": torch.tensor([csteps], dtype=torch.float32, device=dev),
                      "coef_scratch": torch.zeros(64, dtype=torch.float32, device=dev),
                      "pd_inverse": _E.pde_desc(self.pde.KIND, self.pde.dimension, [], self.pde._loss_function_name(),
                                                self.pde._huber_delta())})
        F = self._flat
        learned = getattr(self.pde, "learned", None)
        if learned is not None:
            # a term system with `learn`: its (P,) parameter tensor IS the buffer the kernel reads, so it stays where it is; beside
            # it its own Adam moments and step counter (those of eager steps taken so far come along), and a slice of the gradient
            # buffer behind the loss sum that the residual launch writes d loss / d parameters into
            P = int(learned.numel())
            self.pde.coef_values  # places `learned` on the PDE's device
            lm, lv = torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.float32, device=dev)
            lsteps = 0.0
            st = self.optimizer.state.get(learned, {})
            if "exp_avg" in st:
                lm.copy_(st["exp_avg"].reshape(-1))
                lv.copy_(st["exp_avg_sq"].reshape(-1))
                lsteps = float(st["step"])
            F["grad"] = torch.zeros(n + 4 + 8, dtype=torch.float32, device=dev)  # [gradient | loss sum, pad | parameter gradients]
            F.update({"learn": learned.data, "learn_m": lm, "learn_v": lv, "learn_grad": F["grad"][n + 4 : n + 4 + P],
                      "learn_step": torch.tensor([lsteps], dtype=torch.float32, device=dev),
                      "learn_scratch": torch.zeros(64, dtype=torch.float32, device=dev)})
        F["extra"] = torch.zeros(2, dtype=torch.float32, device=dev)  # {initial, data} when the chain carries a data term
        if self._causal is not None:
            # causal weighting: the sharpness as a device scalar (read at launch time: `set_causal_eps`), the bin means and
            # weights of the last step and the partial sums of pinn_causal_weights
            M, eps = self._causal
            F.update({"causal_host": (M, eps), "causal_eps": torch.tensor([eps], dtype=torch.float32, device=dev),
                      "causal_losses": torch.zeros(M, dtype=torch.float32, device=dev),
                      "causal_w": torch.ones(M, dtype=torch.float32, device=dev),
                      "causal_scratch": torch.zeros(PINN_CAUSAL_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)})
        if self.pde._manual_smoothness() is not None:
            F["smooth_loss"] = torch.zeros(1, dtype=torch.float32, device=dev)  # the unweighted smoothness term of the last step
        if self.use_adaptive_weights:
            # adaptive loss weights: one gradient row per component [residual, boundary, initial] and the EMA state of
            # pinn_adaptive_adam_step {running[4], prev_weights[4], weights[4], calls, has_prev}; the state of eager steps
            # taken so far (`_EmaLossWeights`) comes along
            aw = self.adaptive_weights
            state = torch.zeros(16, dtype=torch.float32)
            if aw.running is not None:
                state[0:3] = aw.running.detach().float().cpu()[:3]
                state[8:11] = aw.weights.detach().float().cpu()[:3]
                state[12] = 1.0
                if aw.prev_weights is not None:
                    state[4:7] = aw.prev_weights.detach().float().cpu()[:3]
                    state[13] = 1.0
            F.update({"comp_grads": torch.zeros(3, n, dtype=torch.float32, device=dev), "aw_state": state.to(dev),
                      "weights": state[8:12].clone().to(dev),
                      "aw_scratch": torch.zeros(PINN_ADAPTIVE_SCRATCH_FLOATS, dtype=torch.float32, device=dev)})
        return self._flat

    def _chain(self, n_batch: int, world: int = 1):
        """The boundary / initial part of `compute_loss` as a launch-list description (`PDEBase._manual_chain`: fixed
        evaluation points, stream set, loss terms), cached per batch length (HeatEquation sizes its point sets from it
        when the config carries no counts) with its persistent buffers."""
        F = self._flat
        key = (int(n_batch), int(world))
        ch = F["chains"].get(key)
        if ch is None:
            ch = dict(self.pde._manual_chain(int(n_batch)))
            dev = self.device
            obs = getattr(self.pde, "observation_data", None)
            ch["has_data"] = bool(ch.get("n_data"))  # a term system's `observations`: its chain carries the data terms already
            ch.setdefault("n_data", 1)
            if obs and self.pde._training_mode() in ("inverse", "data_augmented"):
                # the data term l(model(obs) - u_obs) (pde_base.py:281-291): one more point range and one more term of the chain
                dw = self.pde._data_loss_weight(1.0)
                if dw <= 0.0:
                    dw = 1.0
                if len(ch["terms"]) + 1 > 8:
                    raise NotImplementedError("more than 8 loss terms in the boundary / initial / data chain")
                lo = ch["x"].shape[0]
                xo = obs["x"].to(dev).float().reshape(-1, ch["x"].shape[1])
                to = obs["t"].to(dev).float().reshape(-1, 1)
                ch["x"] = torch.cat([ch["x"], xo], 0).contiguous()
                ch["t"] = torch.cat([ch["t"], to], 0).contiguous()
                ch["terms"] = list(ch["terms"]) + [(lo, lo + xo.shape[0], 0, 0, obs["u"].to(dev).float().reshape(-1).contiguous(), float(dw))]
                ch["has_data"] = True
            # a system's chain ("components" = C): the value rows of its C component forwards, stacked, are the (C, n) block
            K, npts = ch.get("components") or (1 + ch["nt"] + ch["nx"]), ch["x"].shape[0]
            ch["term_losses"] = torch.zeros(len(ch["terms"]), dtype=torch.float32, device=dev)
            ch["cot"] = torch.zeros(K, npts, dtype=torch.float32, device=dev)
            if "face" in ch:
                self._face_buffers(ch)
            ch["terms_dp"] = [(lo, hi, st, pr, tg, w / world) for lo, hi, st, pr, tg, w in ch["terms"]]
            if self.use_adaptive_weights:
                # the boundary and the initial component separately, unweighted (the weights are the adaptive ones):
                # pinn_jet_losses overwrites its cotangents, so each half has its own buffers
                unit = [(lo, hi, st, pr, tg, 1.0) for lo, hi, st, pr, tg, w in ch["terms"]]
                for half, terms in (("b", unit[: ch["n_bc"]]), ("i", unit[ch["n_bc"]:])):
                    ch["terms_" + half] = terms
                    ch["term_losses_" + half] = torch.zeros(len(terms), dtype=torch.float32, device=dev)
                    ch["cot_" + half] = torch.zeros(K, npts, dtype=torch.float32, device=dev)
                    ch["summary_" + half] = torch.zeros(4, dtype=torch.float32, device=dev)
            if "causal_eps" in F:
                ch["causal_cot"] = torch.zeros(int(n_batch), dtype=torch.float32, device=dev)  # the residual's cotangents
            sm = self.pde._manual_smoothness()
            if sm is not None:
                # the finite-difference smoothness term on the collocation batch: its 3 n_batch stencil points, the
                # cotangents of their values and the partial sums of pinn_fd_smoothness
                nb = int(n_batch)
                ch["smooth"] = dict(sm, x3=torch.zeros(3 * nb, 1, dtype=torch.float32, device=dev),
                                    t3=torch.zeros(3 * nb, 1, dtype=torch.float32, device=dev),
                                    cot3=torch.zeros(1, 3 * nb, dtype=torch.float32, device=dev),
                                    scratch=torch.zeros(PINN_FD_SCRATCH_DOUBLES, dtype=torch.float64, device=dev))
            F["chains"][key] = ch
        return ch

    def _face_buffers(self, ch):
        """The buffers of a chain with per-face conditions (`FaceConditions.chain`): ONE jets buffer that every launch of the
        chain writes its rows into, launch after launch, a cotangent buffer of the same layout (zeroed here, once: pinn_face_losses
        writes exactly the floats its terms name, so a row no term reads — u_t of a (1, 1) launch — stays zero), the table with
        its segments as offsets in floats, the term losses and the scratch of pinn_face_losses."""
        dev, face = self.device, ch["face"]
        base, views = 0, []
        for lo, hi, nt, nx, axis, comp in face["launches"]:
            views.append((base, 1 + nt + nx, hi - lo))
            base += (1 + nt + nx) * (hi - lo)
        jets = torch.zeros(base, dtype=torch.float32, device=dev)
        cot = torch.zeros(base, dtype=torch.float32, device=dev)
        table = []
        for tm in face["terms"]:
            e = dict(tm)
            for name in ("value", "value_pair", "deriv", "deriv_pair"):
                if tm.get(name) is not None:
                    launch, row, first = tm[name]
                    b, _, npts = views[launch]
                    e[name] = b + row * npts + first
            table.append(e)
        ch["face_jets"], ch["face_cot"] = jets, cot
        ch["face_views"] = [(ch["x"][lo:hi], ch["t"][lo:hi], jets[b : b + K * n].view(K, n), cot[b : b + K * n].view(K, n))
                            for (lo, hi, *_), (b, K, n) in zip(face["launches"], views)]
        ch["face_table"] = _E.FaceTerms(table)
        ch["term_losses"] = torch.zeros(len(table), dtype=torch.float32, device=dev)
        ch["face_scratch"] = torch.zeros(PINN_FACE_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)

    def _manual_launches(self, x, t, side=None):
        """One optimiser step as a fixed launch sequence, no autograd (pinnrl/training/trainer.py:686-698 with
        pinnrl/pdes/pde_base.py:1086-1235 inlined): zero the flat gradient; residual + mean l(r) + d/dtheta in one
        launch; network values on the 200 boundary + 100 initial points; their loss terms and cotangents; their
        reverse sweep (`_loss_grad_launches`, which is also the closure of the flat L-BFGS); clip_grad_norm_ + Adam over
        the flat buffers.

        `side`: a second stream for the boundary / initial chain (forward, loss terms, reverse sweep into its own
        gradient buffer).  The residual launch leaves most CUs idle during its last tile round (1 555 tiles on 256 CUs:
        19 CUs run a seventh tile), which is where the side chain's 10 tiles then run; the two gradients are added
        after the join, so no two launches ever write the same buffer concurrently."""
        F = self._flat
        prog = self.model.program()
        pd = None if "coef" in F else self.pde._pde_desc()  # trainable coefficients are never read on the host
        n, N = F["n"], x.shape[0]
        loss_name, delta = self.pde._loss_function_name(), self.pde._huber_delta()
        if self.process_group is not None:
            return self._manual_launches_dp(x, t, F, prog, pd, n, N, loss_name, delta)

        ch = self._chain(N)
        if self.use_adaptive_weights:
            return self._manual_launches_adaptive(x, t, F, prog, pd, ch, side)
        self._loss_grad_launches(x, t, F, prog, pd, ch, side)
        _E.adam_clip_step(F["theta"], F["grad"], F["m"], F["v"], F["lr"], F["step"], F["scratch"], beta1=F["betas"][0],
                          beta2=F["betas"][1], eps=F["eps"], weight_decay=F["wd"],
                          max_norm=float(self.config.training.gradient_clipping))
        if "coef" in F:
            # the reference clips model.parameters() only (trainer.py:690-694) and steps everything with one Adam: the same
            # update rule on the trainable coefficient slice, unclipped, with its own step counter
            lo, hi = F["coef_slice"]
            _E.adam_clip_step(F["coef"][lo:hi], F["coef_grad"][lo:hi], F["coef_m"][lo:hi], F["coef_v"][lo:hi], F["lr"],
                              F["coef_step"], F["coef_scratch"], beta1=F["betas"][0], beta2=F["betas"][1], eps=F["eps"],
                              weight_decay=F["wd"], max_norm=0.0)
        if "learn" in F:  # the same rule for the learnable parameters of a term system: unclipped, the shared lr
            _E.adam_clip_step(F["learn"], F["learn_grad"], F["learn_m"], F["learn_v"], F["lr"], F["learn_step"], F["learn_scratch"],
                              beta1=F["betas"][0], beta2=F["betas"][1], eps=F["eps"], weight_decay=F["wd"], max_norm=0.0)

    def _loss_grad_launches(self, x, t, F, prog, pd, ch, side=None):
        """The launch list up to, but not including, its optimiser tail: leaves [flat gradient || loss sum] in F["grad"] and
        {residual, boundary, initial, total} in F["summary"].  The Adam step runs it once; an L-BFGS step runs it once per
        closure evaluation."""
        n, N = F["n"], x.shape[0]
        loss_name, delta = self.pde._loss_function_name(), self.pde._huber_delta()

        def residual_launch():
            causal = self._causal
            if causal is not None:
                # causal weighting: the residual field, its time-bin weights and weighted cotangents (the loss sum lands
                # where the fused launch leaves it), the reverse sweep of the residual
                self._sync_causal_state(F, causal)
                r, _ = _E.residual_forward(prog, pd, x, t, want_loss_sum=False)
                td = self.pde.time_domain
                _E.causal_weights(r.reshape(-1), t.detach().float().contiguous().reshape(-1), causal[0], td[0], td[1],
                                  F["causal_eps"], loss_name, delta, F["rw"] / float(N), loss_sum=F["grad"][n : n + 1],
                                  cot=ch["causal_cot"], bin_losses=F["causal_losses"], bin_weights=F["causal_w"],
                                  scratch=F["causal_scratch"])
                _E.residual_backward(prog, pd, x, t, ch["causal_cot"], F["grad"][:n])
                return
            if "coef" in F:  # trainable coefficients: read from the device buffer, cotangents into their gradient slots
                _E.residual_loss_grad_inverse(prog, F["pd_inverse"], F["coef"], x, t, F["rw"] / float(N), F["grad"][:n],
                                              F["coef_grad"], loss_sum=F["grad"][n : n + 1])
            elif "learn" in F:  # a term system with `learn`: the parameter gradients from the same element-wise launch
                _E.residual_loss_grad(prog, pd, x, t, F["rw"] / float(N), F["grad"][:n], loss_sum=F["grad"][n : n + 1],
                                      param_grads=F["learn_grad"])
            else:
                _E.residual_loss_grad(prog, pd, x, t, F["rw"] / float(N), F["grad"][:n], loss_sum=F["grad"][n : n + 1])

        C = ch.get("components", 0)  # a system: one component launch per field, its value row the stream of that field
        face = ch.get("face")  # per-face conditions: value and derivative launches into one buffer, pinn_face_losses

        def face_losses(summary):
            _E.face_losses(ch["face_jets"], ch["face_table"], loss_name, delta, ch["term_losses"], ch["face_cot"], ch["face_scratch"],
                           residual_sum=F["grad"][n : n + 1] if summary else None, residual_scale=1.0 / float(N),
                           residual_weight=F["rw"], n_boundary_terms=ch["n_bc"], summary4=F["summary"] if summary else None)

        def boundary_chain(grad, summary):
            if face is not None:
                for (lo, hi, nt, nx, axis, comp), (xv, tv, jv, cv) in zip(face["launches"], ch["face_views"]):
                    _E.jets_forward(prog, xv, tv, nt, nx, axis=axis, component=comp, out=jv)
                face_losses(summary)
                for (lo, hi, nt, nx, axis, comp), (xv, tv, jv, cv) in zip(face["launches"], ch["face_views"]):
                    _E.jets_backward(prog, xv, tv, nt, nx, cv, grad, axis=axis, component=comp)
                return ch["face_jets"]
            if C:
                u = torch.cat([_E.jets_forward(prog, ch["x"], ch["t"], 0, 0, component=c) for c in range(C)], 0)
            else:
                u = _E.jets_forward(prog, ch["x"], ch["t"], ch["nt"], ch["nx"])
            _E.jet_losses(u, ch["terms"], loss_name, delta, ch["term_losses"], ch["cot"],
                          residual_sum=F["grad"][n : n + 1] if summary else None, residual_scale=1.0 / float(N),
                          residual_weight=F["rw"], n_boundary_terms=ch["n_bc"], summary4=F["summary"] if summary else None)
            if C:
                for c in range(C):
                    _E.jets_backward(prog, ch["x"], ch["t"], 0, 0, ch["cot"][c : c + 1], grad, component=c)
            else:
                _E.jets_backward(prog, ch["x"], ch["t"], ch["nt"], ch["nx"], ch["cot"], grad)
            return u

        F["grad"].zero_()
        if side is None:
            residual_launch()
            boundary_chain(F["grad"][:n], True)
        else:
            main = torch.cuda.current_stream(self.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                F["grad_side"].zero_()
                u = boundary_chain(F["grad_side"], False)
            residual_launch()
            main.wait_stream(side)
            if not torch.cuda.is_current_stream_capturing():
                u.record_stream(main)
            F["grad"][:n].add_(F["grad_side"])
            # the {residual, boundary, initial, total} summary needs the residual launch's loss sum: the (3 us) loss-term
            # kernel runs once more here; it rewrites the same cotangents
            if face is not None:
                face_losses(True)
            else:
                _E.jet_losses(u, ch["terms"], loss_name, delta, ch["term_losses"], ch["cot"], residual_sum=F["grad"][n : n + 1],
                              residual_scale=1.0 / float(N), residual_weight=F["rw"], n_boundary_terms=ch["n_bc"],
                              summary4=F["summary"])
        sm = ch.get("smooth")
        if sm is not None:
            # the smoothness term (HeatEquation._compute_smoothness_loss), after the summary is written and every other
            # gradient is in place: stencil points of the batch, their values, S + cotangents (total += weight * S), the
            # reverse sweep into the same flat gradient.  On the main stream, after the join: nothing else writes
            # F["grad"] or F["summary"] by then.  The term does not depend on the PDE coefficients.
            _E.fd_stencil_points(x.detach().float().contiguous().reshape(-1), t.detach().float().contiguous().reshape(-1),
                                 sm["eps"], sm["lo"], sm["hi"], sm["x3"], sm["t3"])
            u3 = _E.jets_forward(prog, sm["x3"], sm["t3"], 0, 0)
            _E.fd_smoothness(u3, sm["eps"], sm["weight"], F["smooth_loss"], sm["cot3"], sm["scratch"], summary4=F["summary"])
            _E.jets_backward(prog, sm["x3"], sm["t3"], 0, 0, sm["cot3"], F["grad"][:n])
        F["has_data"] = ch["has_data"]
        if ch["has_data"]:
            # summary4's `initial` is "all terms after the boundary ones": split the data terms (the last ones) out of it
            tl = ch["term_losses"]
            nd = int(ch["n_data"])
            F["extra"][0:1].copy_(tl[ch["n_bc"] : tl.numel() - nd].sum(0, keepdim=True))
            F["extra"][1:2].copy_(tl[tl.numel() - nd :].sum(0, keepdim=True))

    def _manual_launches_adaptive(self, x, t, F, prog, pd, ch, side=None):
        """The launch list with adaptive loss weights (RBW / LRW, trainer.py:586-684).  The weights are detached numbers, so
        grad(total) = sum_c w_c grad(L_c): the residual launch (scale 1/N) writes row 0 of the component gradients, the
        boundary and the initial half of the chain rows 1 and 2 (one forward, two loss-term launches with unit weights, two
        ten-tile reverse sweeps), and `pinn_adaptive_adam_step` does the rest on the device — Gram matrix of the rows (LRW's
        norms, the clip norm), the EMA rule, combine + clip + Adam.  The same path serves both strategies; nothing is read
        on the host, so the step is capturable.  Like the eager `_adaptive_total`, and unlike the reference's LRW branch
        (which leaves the last component's gradient in `.grad` when `loss.backward()` runs), the update uses grad(total) alone."""
        n, N = F["n"], x.shape[0]
        loss_name, delta = self.pde._loss_function_name(), self.pde._huber_delta()
        G = F["comp_grads"]

        def chain():
            u = _E.jets_forward(prog, ch["x"], ch["t"], ch["nt"], ch["nx"])
            _E.jet_losses(u, ch["terms_b"], loss_name, delta, ch["term_losses_b"], ch["cot_b"],
                          n_boundary_terms=len(ch["terms_b"]), summary4=ch["summary_b"])  # summary_b[1] = boundary loss
            _E.jet_losses(u, ch["terms_i"], loss_name, delta, ch["term_losses_i"], ch["cot_i"],
                          n_boundary_terms=0, summary4=ch["summary_i"])  # summary_i[2] = initial loss
            _E.jets_backward(prog, ch["x"], ch["t"], ch["nt"], ch["nx"], ch["cot_b"], G[1])
            _E.jets_backward(prog, ch["x"], ch["t"], ch["nt"], ch["nx"], ch["cot_i"], G[2])
            return u

        G.zero_()
        F["grad"][n:].zero_()  # the residual launch's loss sum stays where the fixed-weight step keeps it
        if side is None:
            _E.residual_loss_grad(prog, pd, x, t, 1.0 / float(N), G[0], loss_sum=F["grad"][n : n + 1])
            chain()
        else:  # the chain beside the residual launch, as in the fixed-weight step: the rows are disjoint buffers
            main = torch.cuda.current_stream(self.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                u = chain()
            _E.residual_loss_grad(prog, pd, x, t, 1.0 / float(N), G[0], loss_sum=F["grad"][n : n + 1])
            main.wait_stream(side)
            if not torch.cuda.is_current_stream_capturing():
                u.record_stream(main)
        F["has_data"] = False
        aw = self.config.training.adaptive_weights
        _E.adaptive_adam_step(F["theta"], G, [F["grad"][n : n + 1], ch["summary_b"][1:2], ch["summary_i"][2:3]], F["m"], F["v"],
                              F["lr"], F["step"], F["aw_scratch"], F["aw_state"], strategy=aw.strategy,
                              alpha=float(aw.alpha), aw_eps=float(aw.eps), initial_weights=aw.initial_weights,
                              loss_scales=[1.0 / float(N), 1.0, 1.0], weights_out=F["weights"], summary4=F["summary"],
                              beta1=F["betas"][0], beta2=F["betas"][1], eps=F["eps"], weight_decay=F["wd"],
                              max_norm=float(self.config.training.gradient_clipping))

    def _manual_launches_dp(self, x, t, F, prog, pd, n, N, loss_name, delta):
        """The same launch list under a process group (one process per GPU): this rank's contiguous shard of the
        identically-sampled batch goes through the residual launch with the GLOBAL 1/N, the replicated boundary /
        initial chain contributes with weight 1/world, ONE in-place sum all-reduce carries [flat gradient || residual
        loss sum], and every rank applies the same clip + Adam update: replicas stay bit-identical."""
        pg = self.process_group
        world = torch.distributed.get_world_size(pg)
        xs, ts, _ = _D.shard_points(x, t, pg)
        ch = self._chain(N, world)
        F["grad"].zero_()
        _E.residual_loss_grad(prog, pd, xs, ts, F["rw"] / float(N), F["grad"][:n], loss_sum=F["grad"][n : n + 1])
        u = _E.jets_forward(prog, ch["x"], ch["t"], ch["nt"], ch["nx"])
        _E.jet_losses(u, ch["terms_dp"], loss_name, delta, ch["term_losses"], ch["cot"])
        _E.jets_backward(prog, ch["x"], ch["t"], ch["nt"], ch["nx"], ch["cot"], F["grad"][:n])
        torch.distributed.all_reduce(F["grad"], op=torch.distributed.ReduceOp.SUM, group=pg)
        # loss terms with the unscaled weights and the reduced (global) residual sum, for the step's summary
        _E.jet_losses(u, ch["terms"], loss_name, delta, ch["term_losses"], ch["cot"], residual_sum=F["grad"][n : n + 1],
                      residual_scale=1.0 / float(N), residual_weight=F["rw"], n_boundary_terms=ch["n_bc"], summary4=F["summary"])
        _E.adam_clip_step(F["theta"], F["grad"], F["m"], F["v"], F["lr"], F["step"], F["scratch"], beta1=F["betas"][0],
                          beta2=F["betas"][1], eps=F["eps"], weight_decay=F["wd"],
                          max_norm=float(self.config.training.gradient_clipping))

    def _manual_losses(self, static: bool = False):
        """{residual, boundary, initial, total} of the last manual step — with a smoothness term on the launch list also
        "smoothness" (unweighted; it is part of total); with adaptive loss weights also "weights", the
        step's four weights (padded with 0), and total = sum_c w_c L_c.  `static=True` hands out views of the persistent
        summary buffer (what a captured graph refreshes in place); otherwise independent copies, so that a caller may
        keep one per step (`train()` averages them per epoch)."""
        s = self._flat["summary"]
        e = self._flat["extra"]
        if not static:
            s, e = s.clone(), e.clone()
        out = {"residual": s[0], "boundary": s[1], "initial": s[2], "total": s[3]}
        if self._flat.get("has_data"):
            out["initial"], out["data"] = e[0], e[1]
        elif self.pde._training_mode() in ("inverse", "data_augmented"):
            out["data"] = torch.zeros((), dtype=torch.float32, device=s.device)
        if "smooth_loss" in self._flat:
            out["smoothness"] = self._flat["smooth_loss"][0] if static else self._flat["smooth_loss"][0].clone()
        if "weights" in self._flat:
            out["weights"] = self._flat["weights"] if static else self._flat["weights"].clone()
        return out

    def _flush_loss_weights(self):
        """`history["loss_weights"]` rows of the launch-list steps taken since the last flush: `train_step` keeps device
        copies (no host sync per step), this converts them where the host waits for the device anyway."""
        if self._pending_weights:
            self.history["loss_weights"].extend(torch.stack(self._pending_weights).double().cpu().numpy())
            self._pending_weights.clear()

    def get_training_history(self):  # trainer.py:966-972
        self._flush_loss_weights()
        return self.history

    def make_graphed_step(self, batch_size: int, warmup: int = 2):
        """Capture ONE whole training step in a HIP graph and return `(replay, losses)`: `replay()` runs a step on a
        fresh device-side sample, `losses` is the dict of STATIC loss tensors it refreshes.

        The captured step contains no autograd at all: it is `_manual_launches` — a handful of kernels of this library (the boundary /
        initial chain forked onto a second stream beside the residual launch) plus the sampler's element-wise ones — writing into persistent flat buffers (parameters, gradient, Adam
        moments; the parameters of the model become views of the flat buffer).  Nothing in it depends on autograd
        nodes of earlier eager steps, so it is safe to call after any number of `train_step`s (round 1's capture of
        `loss.backward()` crashed on a stale AccumulateGrad node).  The learning rate lives in a device scalar that
        `train` refreshes after each scheduler step.  Adaptive loss weights (RBW / LRW) of a forward problem are part of
        the captured step (`_manual_launches_adaptive`: the EMA state lives on the device; `losses["weights"]` is the
        static 4-vector of the last replay).  HeatEquation's finite-difference smoothness term (1-D, fixed loss weights) is
        part of it too: four more launches on the main stream after the join (`losses["smoothness"]` is the static,
        unweighted term of the last replay).  With causal weighting the residual launch is the chain forward ->
        `pinn_causal_weights` -> reverse on the main stream; a replay follows `set_causal_eps`, and `causal_weights()` is the
        static weight vector of the last replay.  Steps the fixed sequence does not cover (`_manual_step_unsupported()`:
        L-BFGS, adaptive weights in inverse / data modes or with a smoothness component, >= 2-D problems other than a
        `TermPDEnD`, data-parallel training) raise."""
        why = self._manual_step_unsupported()
        if why is None and (self._is_lbfgs or getattr(self.config.training, "optimizer", "adam") != "adam"):
            why = "L-BFGS: its line search decides on the host"
        if why is None and self.process_group is not None:
            why = "data-parallel training (a collective inside the capture)"
        if why is not None:
            raise NotImplementedError(f"graph capture covers the plain Adam step only ({why})")
        self._build_flat_state()

        overlap = torch.cuda.Stream(device=self.device)  # boundary / initial chain, forked and joined inside the step

        def step():
            x, t = self._sample(batch_size)
            self._manual_launches(x, t, side=overlap)

        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 1)):  # sizes the engine's scratch (both streams) and the allocator pools before capture
                step()
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        self._step_graph = graph  # keeps the captured allocations alive
        return graph.replay, self._manual_losses(static=True)

    def set_causal_eps(self, value: float) -> None:
        """Set the sharpness of the causal weighting (finite, >= 0): written into the training config the PDE reads, which
        is where the autograd step and the eager launch list take it from, and in place into the launch list's device
        scalar, so a captured step follows it from its next replay.  A captured step follows no other way of changing it."""
        causal = self._causal
        if causal is None:
            raise RuntimeError("set_causal_eps: training.causal_weighting is not enabled")
        eps = validate_causal_eps(value)
        cw = self.pde._training_attr("causal_weighting", None)
        if isinstance(cw, dict):
            cw["eps"] = eps
        else:
            cw.eps = eps
        F = getattr(self, "_flat", None)
        if F is not None and "causal_eps" in F:
            F["causal_eps"].fill_(eps)
            F["causal_host"] = (F["causal_host"][0], eps)

    def causal_weights(self) -> torch.Tensor:
        """The (num_bins,) weights of the causal residual loss: on the launch list those of the last step; on the autograd
        path those of the PDE's last `compute_loss`, a validation pass included.  Ones before the first evaluation.  The last
        entry is the convergence indicator of causal training: it approaches 1 as the residual is resolved over the whole
        time domain."""
        causal = self._causal
        if causal is None:
            raise RuntimeError("causal_weights: training.causal_weighting is not enabled")
        F = getattr(self, "_flat", None)
        if F is not None and "causal_w" in F:
            return F["causal_w"]
        last = getattr(self.pde, "_causal_last_weights", None)
        return last if last is not None else torch.ones(causal[0], dtype=torch.float32, device=self.device)

    def set_learning_rate(self, lr: float) -> None:
        """Propagate a scheduler's learning rate to the device scalar the captured / manual step reads."""
        if getattr(self, "_flat", None) is not None:
            self._flat["lr"].fill_(float(lr))

    # ---------------------------------------------------------------- the loop (trainer.py:391-964)
    def train(self, num_epochs: int, batch_size: int, num_points: int, experiment_dir: str = None):
        self.model.train()
        if self._is_lbfgs and batch_size != num_points:
            batch_size = num_points  # L-BFGS needs full-batch closures (trainer.py:455-461)
        if getattr(self, "_flat", None) is None and self.fast_step is not False:
            why = self._manual_step_unsupported()
            if why is None and torch.device(self.device).type == "cuda":
                self._build_flat_state()  # from here on `train_step` is the fixed launch list (no autograd)
            elif self.fast_step:
                raise NotImplementedError(f"fast_step=True, but the autograd-free step does not cover this configuration ({why})")
        trainable = dict(getattr(self.pde, "_trainable_params", {}))
        for name in trainable:
            self.history.setdefault(f"param_{name}", [])
        start = datetime.now()
        for epoch in range(num_epochs):
            self.model.train()
            step_losses = []
            losses = None
            for _ in range(num_points // batch_size):
                x, t = self._sample(batch_size)
                losses = self.train_step(x, t)
                step_losses.append(losses["total"].detach().clone())  # the manual step's losses may alias one buffer
                if self.log_every_step:
                    self.points_history.append(torch.cat([x, t], dim=1).cpu().numpy())
            avg = float(torch.stack(step_losses).mean().item())  # ZeroDivisionError upstream when there are no steps
            self._flush_loss_weights()
            self._update_scheduler(avg)
            lr = self.optimizer.param_groups[0]["lr"]
            self.set_learning_rate(lr)
            row = {"train_loss": avg, "residual_loss": float(losses["residual"]), "boundary_loss": float(losses["boundary"]),
                   "initial_loss": float(losses["initial"]), "learning_rate": lr}
            if "data" in losses:
                self.history.setdefault("data_loss", [])
                row["data_loss"] = float(losses["data"])
            for name, p in trainable.items():
                row[f"param_{name}"] = float(p.detach().cpu().item())
            for k, v in row.items():
                if k in self.history:
                    self.history[k].append(v)
            if experiment_dir and self.viz_frequency and epoch % self.viz_frequency == 0:
                self._save_live_snapshot(experiment_dir, epoch)
            if epoch % self.validation_frequency == 0:
                val = self._compute_validation_loss()
                self.history["val_loss"].append(val["total_loss"])
                if self.early_stopping_enabled:
                    if val["total_loss"] < self.best_val_loss - 1e-6:
                        self.best_val_loss, self.patience_counter = val["total_loss"], 0
                    else:
                        self.patience_counter += 1
                    if self.patience_counter >= self.patience:
                        self.logger.info(f"Early stopping triggered at epoch {epoch + 1}")
                        break
            if (self._optimizer_type == "adam_lbfgs" and not self._is_lbfgs and self._switch_epoch is not None
                    and (epoch + 1) >= self._switch_epoch):
                self._switch_to_lbfgs()
                batch_size = num_points
        self.training_time_minutes = (datetime.now() - start).total_seconds() / 60.0
        return self.history
