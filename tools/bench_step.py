"""Full training step (SURVEY §8(d) "secondary: full-step pts/s", §8(f) rank 1) on ONE GPU, for context.

    python tools/bench_step.py [--configs C1,C2,C3,C4] [--steps 30] [--modes autograd,manual,graph]
                               [--adaptive {none,rbw,lrw}] [--repeats 1] [--optimizer {adam,lbfgs}] [--smoothness W]
                               [--term-pde] [--term-nd] [--term-mixed] [--causal M,EPS]
                               [--system {gray_scott,navier_stokes,elasticity,elasticity_nomixed,navier_stokes_forced,
                                          advection_diffusion,euler_nl,navier_stokes_inverse}]

One step = fresh collocation sample (the configuration's own sampler: uniform, or the DQN-adaptive sampler for C3) ->
residual + boundary + initial loss terms -> gradient -> clip_grad_norm_ -> Adam, i.e. the reference's inner loop
(pinnrl/training/trainer.py:546-698), at the BASELINE configurations' full sizes:

    autograd  `PDETrainer.train_step` with torch autograd around the fused launches (the reference's call sequence)
    manual    the autograd-free launch list (`_manual_launches`: what `PDETrainer.train()` takes by itself)
    graph     the same list captured once in a HIP graph (`make_graphed_step`) and replayed

`--adaptive rbw|lrw` turns on adaptive loss weights (`training.adaptive_weights`, default settings of the configuration):
the autograd mode then runs `_adaptive_total` (LRW: one backward pass per loss component), the other two the adaptive launch
list (`pinn_adaptive_adam_step`).  `--repeats R` times the window R times and prints the median with the range.

`--smoothness W` (C1 only) runs HeatEquation with the reference's default loss weights {residual 15, boundary 20, initial 10,
smoothness W}: its finite-difference smoothness term is three more network evaluations of the batch and their reverse
sweeps — autograd nodes in the autograd mode, four launches of the launch list in the other two.

`--term-pde` (C2 only) runs Burgers as a `TermPDE` (u_t + u u_x - nu u_xx given as three terms): the residual part of the
step is then the chain pinn_jet_forward -> pinn_term_residual -> pinn_jet_backward in place of the one fused launch.  After
the step table it times those three launches on their own (device time between two events, the step's batch) next to the
compiled kind's `pinn_residual_loss_grad`.

`--term-nd` runs N1 and N2 instead of C1..C4: the heat equation u_t - a Laplacian(u) on fourier 4x128 with 49 729 points, in
1-D as a `TermPDE` (the yardstick) and in 2-D as a `TermPDEnD`, whose residual part is one jet launch per space axis in each
sweep around `pinn_term_residual_axes` (the launch along y on the layer-major engine).

`--term-mixed` runs M1, M2 and M3 instead: fourier 4x128 with 49 729 points in 2-D — M1 the heat equation as a `TermPDEnD`
(N2 above, the yardstick), M2 anisotropic diffusion u_t - a u_xx - 2 b u_xy - c u_yy as a `TermPDEMixed` (one more launch pair,
along e_x + e_y on the set (0, 2)), M3 the 2-D Cahn-Hilliard equation written out as ten terms (four launch pairs: x on (1, 4),
y, e_x + e_y and e_x - e_y on (0, 4)).  After the step table it times every launch of each chain on its own (device time
between two events, the step's batch).

`--system gray_scott` runs N1 and S1, `--system navier_stokes` N2 and S2: a coupled system as a `TermPDESystem` on fourier
4x128 (output_dim = the number of fields) with 49 729 points beside the single-field step with the same stream sets — S1
Gray-Scott in 1-D (two fields on the set (1, 2); N1 is one such field), S2 incompressible Navier-Stokes in 2-D ((u, v, p): two
fields on (1, 2) + (0, 2) along y, the pressure on (1, 1) + (0, 1); N2 is one field on (1, 2) + (0, 2)).  Every field is a
component launch on the layer-major engine, which recomputes the trunk.  After the step table it times every launch of the
system's chain on its own, `pinn_term_residual_system` among them.

`--system elasticity` runs S3: 2-D linear elasticity, fields (u, v), u_t = mu Lap u + (lambda + mu) (u_xx + v_xy), v_t = mu Lap v +
(lambda + mu) (u_xy + v_yy), as a `TermPDESystemMixed` on fourier 4x128, Dirichlet faces — per field the launches along x, y and
e_x + e_y.  `--system elasticity_nomixed` runs S4, the yardstick: the same system on `TermPDESystem` with the two mixed terms
dropped (four launches per sweep against six).  After the step table every launch of the chain is timed on its own; for S4 also
`pinn_term_residual_system_mixed` on the same blocks with all pair orders 0, beside `pinn_term_residual_system`: the cost of
the larger LDS footprint.

`--system navier_stokes_forced` runs S2 beside S5, its forced twin: the same Navier-Stokes system with a body force (fx, fy)
(x, y, t) in the two momentum equations, given as known functions (`TermPDESystem(..., functions=...)`): the same launches, the
element-wise kernel `pinn_term_residual_system_fn` and two function evaluations (torch ops) per residual call.
`--system advection_diffusion` runs S6: one field c in 2-D, c_t + a c_x + b c_y - kappa (c_xx + c_yy) with the rotating field
(a, b) = (-(y - 1/2), x - 1/2) and kappa(x, y) as functions.  For S3 the launch table also times `pinn_term_residual_system_fn` on
the same blocks with no function named, beside `pinn_term_residual_system_mixed`.

`--system euler_nl` runs S7 beside S8: 1-D compressible flow in primitive variables (rho, u, p), whose momentum equation
u_t + u u_x + p_x / (2 + rho) names the nonlinear factor 1 / (2 + rho) (`TermPDESystem(..., nonlinear=...)`, the element-wise
kernel `pinn_term_residual_system_nl`), and S7, its twin with the same nine terms and the same factor counts in which that
factor is the stream rho itself (`pinn_term_residual_system`).

`--system navier_stokes_inverse` runs S2 beside S9, its inverse twin: the same Navier-Stokes system with the convective
coefficient lam and the viscosity nu learnable (`TermPDESystem(..., learn=...)`, starting off their true values) and velocity
observations on 2 000 seeded points with the pressure hidden (`observations=`): the same launches over 2 000 more fixed points,
the element-wise kernel `pinn_term_residual_system_inv`, which also returns d loss / d (lam, nu), and one more three-launch Adam
step on the two parameters.  `--learned STEPS` then trains S9 for STEPS captured steps and prints the learned values.

`--causal M,EPS` turns on the causal (time-weighted) residual loss (`training.causal_weighting`: M time bins, sharpness
EPS): the autograd mode builds the weighted loss with torch ops on the residual tensor, the other two run the residual part
of the step as the chain pinn_residual_forward -> pinn_causal_weights -> pinn_residual_backward in place of the one fused
launch.  After the step table it times those launches on their own next to `pinn_residual_loss_grad`.

`--optimizer lbfgs` times `optimizer="lbfgs"` instead (C2 and C3 unless --configs is given; max_iter 20, history_size 50,
strong Wolfe, lr 1, one fixed full batch as L-BFGS wants it, uniform points): the eager step (torch.optim.LBFGS around an
autograd closure) against the launch list (`_lbfgs_step_flat`).  Both run steps until their ring holds 50 pairs before the
clock starts.  Reported per form: ms per `step()`, closure evaluations per step, and ms per closure evaluation timed on its
own (loss + gradient + the one host read that follows it).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import math  # noqa: E402

import bench_configs as B  # noqa: E402
from pinnrl_amd import engine as E  # noqa: E402
from pinnrl_amd import pdes as P  # noqa: E402
from pinnrl_amd.config import AdaptiveWeightsConfig, CausalWeightingConfig, Config, TrainingConfig  # noqa: E402
from pinnrl_amd.pdes import TermPDE  # noqa: E402
from pinnrl_amd.rl import RLAgent  # noqa: E402
from pinnrl_amd.training import PDETrainer  # noqa: E402


BURGERS_TERMS = [(1.0, ("u_t",)), (1.0, ("u", "u_x")), ((-1.0, "nu"), ("u_xx",))]


def _heat_terms(axes):
    return [(1.0, ("u_t",))] + [((-1.0, "alpha"), (f,)) for f in ("u_xx", "u_yy", "u_zz")[:axes]]


def _heat_nd(dim):
    """Heat equation with the Laplacian of `dim` space dimensions on fourier 4x128, 49 729 points: dim 1 as a `TermPDE` (the
    yardstick: one jet launch per sweep), dim 2 as a `TermPDEnD` (one more launch per sweep along y, on the layer-major engine)."""
    net = B.model("fourier", 128, 4, "tanh", input_dim=dim + 1)
    pc = P.PDEConfig(name="heat", domain=[(0.0, 1.0)] * dim, time_domain=(0.0, 1.0), parameters={"alpha": 0.01},
                     boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}}, initial_condition={"type": "sine"},
                     exact_solution={}, dimension=dim, device=B.dev)
    if dim == 1:
        return "Heat 1D (u_t - a u_xx) as TermPDE, fourier 4x128", net, TermPDE(pc, _heat_terms(1)), 49729
    ic = lambda x: torch.prod(torch.sin(math.pi * x), dim=1)  # noqa: E731
    return f"Heat {dim}D (u_t - a Laplacian u) as TermPDEnD, fourier 4x128", net, P.TermPDEnD(pc, _heat_terms(dim), ic), 49729


ANISO_TERMS = [(1.0, ("u_t",)), ((-1.0, "a"), ("u_xx",)), ((-2.0, "b"), ("u_xy",)), ((-1.0, "c"), ("u_yy",))]
# u_t + eps^2 (u_xxxx + 2 u_xxyy + u_yyyy) - 3 u^2 (u_xx + u_yy) - 6 u (u_x^2 + u_y^2) + u_xx + u_yy
CAHN_HILLIARD_2D_TERMS = [(1.0, ("u_t",)), ((1.0, "eps2"), ("u_xxxx",)), ((2.0, "eps2"), ("u_xxyy",)), ((1.0, "eps2"), ("u_yyyy",)),
                          (-3.0, ("u", "u", "u_xx")), (-3.0, ("u", "u", "u_yy")), (-6.0, ("u", "u_x", "u_x")),
                          (-6.0, ("u", "u_y", "u_y")), (1.0, ("u_xx",)), (1.0, ("u_yy",))]


def _mixed_2d(which):
    """2-D problems with mixed derivatives as `TermPDEMixed` on fourier 4x128, 49 729 points."""
    net = B.model("fourier", 128, 4, "tanh", input_dim=3)
    params, terms, label = {"aniso": ({"a": 0.01, "b": 0.004, "c": 0.02}, ANISO_TERMS, "Anisotropic diffusion 2D (u_t - a u_xx - 2b u_xy - c u_yy)"),
                            "ch": ({"eps2": 1e-4}, CAHN_HILLIARD_2D_TERMS, "Cahn-Hilliard 2D (ten terms)")}[which]
    pc = P.PDEConfig(name=which, domain=[(0.0, 1.0)] * 2, time_domain=(0.0, 1.0), parameters=params,
                     boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}}, initial_condition={"type": "sine"},
                     exact_solution={}, dimension=2, device=B.dev)
    ic = lambda x: torch.prod(torch.sin(math.pi * x), dim=1)  # noqa: E731
    return f"{label} as TermPDEMixed, fourier 4x128", net, P.TermPDEMixed(pc, terms, ic), 49729


GRAY_SCOTT = [[(1.0, ("u_t",)), ((-1.0, "Du"), ("u_xx",)), (1.0, ("u", "v", "v")), ((-1.0, "F"), ()), ((1.0, "F"), ("u",))],
              [(1.0, ("v_t",)), ((-1.0, "Dv"), ("v_xx",)), (-1.0, ("u", "v", "v")), ((1.0, "Fk"), ("v",))]]
NAVIER_STOKES = [
    [(1.0, ("u_t",)), (1.0, ("u", "u_x")), (1.0, ("v", "u_y")), (1.0, ("p_x",)), ((-1.0, "nu"), ("u_xx",)), ((-1.0, "nu"), ("u_yy",))],
    [(1.0, ("v_t",)), (1.0, ("u", "v_x")), (1.0, ("v", "v_y")), (1.0, ("p_y",)), ((-1.0, "nu"), ("v_xx",)), ((-1.0, "nu"), ("v_yy",))],
    [(1.0, ("u_x",)), (1.0, ("v_y",))]]


def _body_force():
    """A smooth body force (fx, fy)(x, y, t) of the forced Navier-Stokes twin: pure device torch ops, so the step captures."""
    fx = lambda x, t: torch.sin(math.pi * x[:, 0]) * torch.cos(math.pi * x[:, 1]) * torch.exp(-t[:, 0])  # noqa: E731
    fy = lambda x, t: -torch.cos(math.pi * x[:, 0]) * torch.sin(math.pi * x[:, 1]) * torch.exp(-t[:, 0])  # noqa: E731
    return {"fx": fx, "fy": fy}


def _advection_diffusion():
    """One field in 2-D, c_t + a c_x + b c_y - kappa (c_xx + c_yy), velocity field and diffusivity as known functions, on fourier
    4x128, 49 729 points, Dirichlet faces."""
    fns = {"a": lambda x, t: -(x[:, 1] - 0.5), "b": lambda x, t: x[:, 0] - 0.5, "kappa": lambda x, t: 0.01 * (1.0 + x[:, 0] * x[:, 1])}
    eqs = [[(1.0, ("c_t",)), (1.0, ("a", "c_x")), (1.0, ("b", "c_y")), (-1.0, ("kappa", "c_xx")), (-1.0, ("kappa", "c_yy"))]]
    net = B.model("fourier", 128, 4, "tanh", input_dim=3, output_dim=1)
    pc = P.PDEConfig(name="advection_diffusion", domain=[(0.0, 1.0)] * 2, time_domain=(0.0, 1.0), parameters={},
                     boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}}, initial_condition={}, exact_solution={},
                     dimension=2, device=B.dev)
    ic = lambda x: torch.exp(-40 * ((x[:, 0] - 0.7) ** 2 + (x[:, 1] - 0.5) ** 2)).unsqueeze(1)  # noqa: E731
    return ("Advection-diffusion 2D (c; a, b, kappa as functions) as TermPDESystem, fourier 4x128", net,
            P.TermPDESystem(pc, ("c",), eqs, ic, functions=fns), 49729)


def _euler(nonlinear):
    """1-D compressible flow in (rho, u, p) on fourier 4x128, 49 729 points, periodic: rho_t + u rho_x + rho u_x,
    u_t + u u_x + F p_x, p_t + u p_x + gamma p u_x with F = 1 / (2 + rho) as a nonlinear factor, or, in the twin, F = rho."""
    F = "ir" if nonlinear else "rho"
    eqs = [[(1.0, ("rho_t",)), (1.0, ("u", "rho_x")), (1.0, ("rho", "u_x"))],
           [(1.0, ("u_t",)), (1.0, ("u", "u_x")), (1.0, (F, "p_x"))],
           [(1.0, ("p_t",)), (1.0, ("u", "p_x")), ((1.0, "gamma"), ("p", "u_x"))]]
    net = B.model("fourier", 128, 4, "tanh", input_dim=2, output_dim=3)
    pc = P.PDEConfig(name="euler_nl" if nonlinear else "euler_twin", domain=[(0.0, 1.0)], time_domain=(0.0, 1.0), parameters={"gamma": 1.4},
                     boundary_conditions={"periodic": {}}, initial_condition={}, exact_solution={}, dimension=1, device=B.dev)
    ic = lambda x: torch.stack([0.2 * torch.sin(2 * math.pi * x[:, 0]), 0.5 * torch.cos(2 * math.pi * x[:, 0]),  # noqa: E731
                                1.0 + 0.1 * torch.sin(2 * math.pi * x[:, 0])], 1)
    label = "Euler 1D (rho, u, p) with 1 / (2 + rho) as a nonlinear factor" if nonlinear else "Euler 1D twin (rho in place of 1 / (2 + rho))"
    return (f"{label} as TermPDESystem, fourier 4x128", net,
            P.TermPDESystem(pc, ("rho", "u", "p"), eqs, ic, nonlinear={"ir": ("recip", "rho", {"shift": 2.0})} if nonlinear else None), 49729)


def _system(which):
    """Coupled systems as `TermPDESystem` on fourier 4x128 with one output per field, 49 729 points."""
    forced = which == "navier_stokes_forced"
    inverse = which == "navier_stokes_inverse"
    if which == "gray_scott":
        fields, eqs, dim, label = ("u", "v"), GRAY_SCOTT, 1, "Gray-Scott 1D (u, v)"
        bcs, ic, icf = {"periodic": {}}, (lambda x: torch.stack([1 - 0.5 * torch.exp(-50 * (x[:, 0] - 0.5) ** 2),
                                                                   0.25 * torch.exp(-50 * (x[:, 0] - 0.5) ** 2)], 1)), None
    else:
        fields, eqs, dim, label = ("u", "v", "p"), NAVIER_STOKES, 2, "Navier-Stokes 2D (u, v, p)"
        if forced:
            eqs = [NAVIER_STOKES[0] + [(-1.0, ("fx",))], NAVIER_STOKES[1] + [(-1.0, ("fy",))], NAVIER_STOKES[2]]
            label = "Navier-Stokes 2D (u, v, p) with a body force (fx, fy as functions)"
        if inverse:  # lam in front of the four convective terms; lam and nu start off their true values 1 and 0.01
            conv = lambda tm: ((1.0, "lam"), tm[1]) if len(tm[1]) == 2 else tm  # noqa: E731
            eqs = [[conv(tm) for tm in NAVIER_STOKES[0]], [conv(tm) for tm in NAVIER_STOKES[1]], NAVIER_STOKES[2]]
            label = "Navier-Stokes 2D (u, v, p), lam and nu learnable, 2 000 velocity observations"
        bcs = {"dirichlet": {"type": "fixed", "value": [0.0, 0.0, None]}}
        ic, icf = (lambda x: torch.stack([torch.sin(math.pi * x[:, 0]) * torch.sin(math.pi * x[:, 1]),
                                          torch.zeros_like(x[:, 0])], 1)), ("u", "v")
    net = B.model("fourier", 128, 4, "tanh", input_dim=dim + 1, output_dim=len(fields))
    pc = P.PDEConfig(name=which, domain=[(0.0, 1.0)] * dim, time_domain=(0.0, 1.0),
                     parameters={"Du": 2e-5, "Dv": 1e-5, "F": 0.04, "Fk": 0.1, "nu": 0.01, "lam": 1.0}, boundary_conditions=bcs,
                     initial_condition={}, exact_solution={}, dimension=dim, device=B.dev)
    extra = {}
    if inverse:
        # velocity data of the decaying Taylor-Green-type field that the initial condition starts: u = e^(-2 pi^2 nu t) sin sin,
        # v = 0 is no Navier-Stokes solution, so the learned values are informational only
        g = torch.Generator().manual_seed(7)
        xo, to = torch.rand(2000, 2, generator=g), torch.rand(2000, 1, generator=g)
        uo = torch.exp(-2 * math.pi**2 * 0.01 * to[:, 0]) * torch.sin(math.pi * xo[:, 0]) * torch.sin(math.pi * xo[:, 1])
        extra = {"learn": {"lam": 0.5, "nu": 0.05},
                 "observations": {"x": xo, "t": to, "u": torch.stack([uo, torch.zeros_like(uo)], 1), "fields": ("u", "v")}}
    return (f"{label} as TermPDESystem, fourier 4x128", net,
            P.TermPDESystem(pc, fields, eqs, ic, initial_condition_fields=icf, functions=_body_force() if forced else None, **extra), 49729)


def _elasticity_equations(mixed):
    eqs = [[(1.0, ("u_t",)), ((-1.0, "mu"), ("u_xx",)), ((-1.0, "mu"), ("u_yy",)), ((-1.0, "a"), ("u_xx",)), ((-1.0, "a"), ("v_xy",))],
           [(1.0, ("v_t",)), ((-1.0, "mu"), ("v_xx",)), ((-1.0, "mu"), ("v_yy",)), ((-1.0, "a"), ("u_xy",)), ((-1.0, "a"), ("v_yy",))]]
    return eqs if mixed else [[tm for tm in eq if not tm[1][0].endswith("_xy")] for eq in eqs]


def _elasticity(mixed):
    """2-D linear elasticity (u, v) on fourier 4x128, 49 729 points, Dirichlet faces: as a `TermPDESystemMixed`, or — the two mixed
    terms dropped — as a `TermPDESystem`."""
    mu, lam = 0.05, 0.08
    kappa = 2 * math.pi**2 * (lam + 2 * mu)

    def exact(x, t):  # (u, v) = grad phi, phi = exp(-kappa t) sin(pi x) sin(pi y): curl-free, so grad div = Laplacian
        e = math.pi * torch.exp(-kappa * t[:, 0])
        return torch.stack([e * torch.cos(math.pi * x[:, 0]) * torch.sin(math.pi * x[:, 1]),
                            e * torch.sin(math.pi * x[:, 0]) * torch.cos(math.pi * x[:, 1])], 1)

    net = B.model("fourier", 128, 4, "tanh", input_dim=3, output_dim=2)
    pc = P.PDEConfig(name="elasticity", domain=[(0.0, 1.0)] * 2, time_domain=(0.0, 1.0), parameters={"mu": mu, "a": lam + mu},
                     boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}}, initial_condition={}, exact_solution={},
                     dimension=2, device=B.dev)
    cls = P.TermPDESystemMixed if mixed else P.TermPDESystem
    ic = lambda x: exact(x, torch.zeros(x.shape[0], 1, device=x.device))  # noqa: E731
    label = "Elasticity 2D (u, v) as TermPDESystemMixed" if mixed else "Elasticity 2D without v_xy, u_xy as TermPDESystem"
    return f"{label}, fourier 4x128", net, cls(pc, ("u", "v"), _elasticity_equations(mixed), ic, exact_solution_fn=exact), 49729


ND_CONFIGS = {"N1": lambda: _heat_nd(1), "N2": lambda: _heat_nd(2),
              "M1": lambda: _heat_nd(2), "M2": lambda: _mixed_2d("aniso"), "M3": lambda: _mixed_2d("ch"),
              "S1": lambda: _system("gray_scott"), "S2": lambda: _system("navier_stokes"),
              "S3": lambda: _elasticity(True), "S4": lambda: _elasticity(False),
              "S5": lambda: _system("navier_stokes_forced"), "S6": _advection_diffusion,
              "S7": lambda: _euler(False), "S8": lambda: _euler(True), "S9": lambda: _system("navier_stokes_inverse")}


def build(tag, adaptive="none", smoothness=0.0, term_pde=False, causal=None):
    name, net, eq, n_req = (ND_CONFIGS.get(tag) or B.CONFIGS[tag])()
    if term_pde:  # the same configuration object, the residual given as data
        eq = TermPDE(eq.config, BURGERS_TERMS)
        name += ", as TermPDE"
    agent = None
    if tag == "C3":  # BASELINE C3: DQN adaptive sampling
        agent = RLAgent(state_dim=2, action_dim=1, hidden_dim=64, device=B.dev)
        eq.rl_agent = agent
    cfg = Config.__new__(Config)
    cfg.device = B.dev
    cfg.training = TrainingConfig()
    if smoothness > 0:  # the reference's default configuration: the PDE reads its loss weights from the training section
        cfg.training = TrainingConfig(loss_weights={"residual": 15.0, "boundary": 20.0, "initial": 10.0, "smoothness": float(smoothness)})
        eq.config.training = cfg.training
        name += f", smoothness {smoothness:g}"
    if adaptive != "none":
        cfg.training.adaptive_weights = AdaptiveWeightsConfig(enabled=True, strategy=adaptive)
    if causal is not None:  # the PDE reads the option from the training section, as it reads the loss function
        cfg.training.causal_weighting = CausalWeightingConfig(enabled=True, num_bins=causal[0], eps=causal[1])
        eq.config.training = cfg.training
        name += f", causal {causal[0]} bins, eps {causal[1]:g}"
    return name, net, eq, agent, cfg, n_req


def bench_lbfgs(args):
    tags = [c for c in args.configs.split(",") if c] if args.configs != "C1,C2,C3,C4" else ["C2", "C3"]
    steps, repeats = max(args.steps, 1), max(args.repeats, 1)
    print("| config | points | form | ms/step() | evaluations/step | ms/evaluation (alone) | last total loss |")
    print("|---|---|---|---|---|---|---|")
    for tag in tags:
        for form in ("eager", "launch list"):
            torch.manual_seed(0)
            name, net, eq, n_req = B.CONFIGS[tag]()
            cfg = Config.__new__(Config)
            cfg.device = B.dev
            cfg.training = TrainingConfig(optimizer="lbfgs", learning_rate=1.0, gradient_clipping=0.0)
            cfg.training.lbfgs.max_iter, cfg.training.lbfgs.history_size = 20, 50
            tr = PDETrainer(net, eq, None, cfg, device=B.dev, fast_step=False)
            if form != "eager":
                why = tr._manual_step_unsupported()
                if why is not None:
                    print(f"| {tag} | - | {form} | not covered: {why} | | | |")
                    continue
                tr._build_flat_state()
            x, t = tr._sample(n_req)
            n = int(x.shape[0])

            def evals(tr=tr, form=form):
                if form == "eager":
                    return tr.optimizer.state[tr.optimizer._params[0]].get("func_evals", 0)
                return tr._flat["lbfgs"]["driver"].func_evals

            def pairs(tr=tr, form=form):
                if form == "eager":
                    return len(tr.optimizer.state[tr.optimizer._params[0]].get("old_dirs", []))
                return int(tr._flat["lbfgs"]["state"][1].item())

            warm = 0
            while warm < 3 or (pairs() < 50 and warm < 10):
                out = tr.train_step(x, t)
                warm += 1
            filled = pairs()
            times, counts = [], []
            for _ in range(repeats):
                e0 = evals()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    out = tr.train_step(x, t)
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0) / steps)
                counts.append((evals() - e0) / steps)
            # one closure evaluation on its own, as the step pays for it: launches + the host read of the loss
            if form == "eager":
                def closure(tr=tr):
                    tr.optimizer.zero_grad()
                    losses = tr._losses(x, t)
                    losses["total"].backward()
                    return float(losses["total"].detach())
            else:
                L = tr._flat["lbfgs"]
                L["batch"] = (x, t)
                closure = lambda L=L: L["driver"].backend.evaluate(None)  # noqa: E731
            for _ in range(3):
                closure()
            ctimes = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    closure()
                torch.cuda.synchronize()
                ctimes.append(1e3 * (time.perf_counter() - t0) / 20)

            def med(v):
                v = sorted(v)
                return f"{v[len(v) // 2]:.3f}" + (f" ({v[0]:.3f}-{v[-1]:.3f})" if len(v) > 1 else "")

            print(f"| {tag} {name} | {n} | {form} (ring {filled}) | {med(times)} | {med(counts)} | {med(ctimes)} | "
                  f"{float(out['total'].detach()):.4e} |", flush=True)
            del tr, net, eq
            torch.cuda.empty_cache()


def time_term_launches(tag, iters=20):
    """Device time of the three launches of the term chain, each on its own, and of the compiled kind's one launch."""
    torch.manual_seed(0)
    name, net, eq, n_req = B.CONFIGS[tag]()
    term = TermPDE(eq.config, BURGERS_TERMS)
    x, t = eq.generate_collocation_points(n_req, strategy="uniform")
    prog, pd, td = net.program(), eq._pde_desc(), term._pde_desc()
    n = int(x.shape[0])
    nt, nx = E.pde_streams(td)
    flat, s = E.new_flat_grad(prog, B.dev), torch.zeros(1, device=B.dev)
    jets = E.jets_forward(prog, x, t, nt, nx)
    _, cot = E.term_residual(td, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True)
    calls = [("pinn_jet_forward", lambda: E.jets_forward(prog, x, t, nt, nx)),
             ("pinn_term_residual (loss sum + cotangents, two launches)",
              lambda: E.term_residual(td, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True)),
             ("pinn_term_residual (residual only, one launch)", lambda: E.term_residual(td, jets, x, t)),
             ("pinn_jet_backward", lambda: E.jets_backward(prog, x, t, nt, nx, cot, flat)),
             ("the chain through engine.residual_loss_grad", lambda: E.residual_loss_grad(prog, td, x, t, 1.0 / n, flat, loss_sum=s)),
             ("compiled kind: pinn_residual_loss_grad", lambda: E.residual_loss_grad(prog, pd, x, t, 1.0 / n, flat, loss_sum=s))]
    print()
    print(f"| {tag} launch ({n} points, kernels {E._lib.kernel_name(prog, n, nt, nx, 0)} / {E._lib.kernel_name(prog, n, nt, nx, 1)}) | ms |")
    print("|---|---|")
    for label, fn in calls:
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"| {label} | {a.elapsed_time(b) / iters:.4f} |", flush=True)


def time_nd_launches(tag, iters=20):
    """Device time of every launch of an n-D term chain on its own: one jet launch per line forward, the element-wise
    residual, one reverse sweep per line."""
    torch.manual_seed(0)
    name, net, eq, n_req = ND_CONFIGS[tag]()
    x, t = eq._sample_uniform(n_req)
    prog, td = net.program(), eq._pde_desc()
    n = int(x.shape[0])
    flat, s = E.new_flat_grad(prog, B.dev), torch.zeros(1, device=B.dev)
    jets = E._axes_jets(prog, td, x, t)
    _, cot = E._term_residual_nd(td, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True)
    calls = []
    for b, (key, nt, nx) in zip(E._launch_blocks(td), td.launches()):
        line = E._launch_line(key)
        calls.append((f"pinn_jet_forward along {key}, set ({nt}, {nx})", lambda nt=nt, nx=nx, line=line: E.jets_forward(prog, x, t, nt, nx, **line)))
        calls.append((f"pinn_jet_backward along {key}, set ({nt}, {nx})",
                      lambda nt=nt, nx=nx, line=line, b=b: E.jets_backward(prog, x, t, nt, nx, cot[b], flat, **line)))
    kind = "mixed" if isinstance(td, E.MixedTermDesc) else "axes"
    calls.append((f"pinn_term_residual_{kind} (loss sum + cotangents, two launches)",
                  lambda: E._term_residual_nd(td, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True)))
    calls.append(("the chain through engine.residual_loss_grad", lambda: E.residual_loss_grad(prog, td, x, t, 1.0 / n, flat, loss_sum=s)))
    print()
    print(f"| {tag} launch ({n} points) | ms |")
    print("|---|---|")
    for label, fn in calls:
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"| {label} | {a.elapsed_time(b) / iters:.4f} |", flush=True)


def time_system_launches(tag, iters=20):
    """Device time of every launch of a system's chain on its own: one component jet launch per (field, axis) — and, with mixed
    derivatives, per (field, direction) — forward, the element-wise residuals of all equations, one component reverse sweep per
    block."""
    torch.manual_seed(0)
    name, net, eq, n_req = ND_CONFIGS[tag]()
    x, t = eq._sample_uniform(n_req)
    prog, td = net.program(), eq._pde_desc()
    n = int(x.shape[0])
    flat, s = E.new_flat_grad(prog, B.dev), torch.zeros(1, device=B.dev)
    jets = E._system_jets(prog, td, x, t)
    entry = ("pinn_term_residual_system_inv" if isinstance(td, E.InvSystemTermDesc) else
             "pinn_term_residual_system_nl" if isinstance(td, E.NlSystemTermDesc) else
             "pinn_term_residual_system_fn + the functions' torch ops" if isinstance(td, E.FnSystemTermDesc) else
             "pinn_term_residual_system_mixed" if isinstance(td, E.MixedSystemTermDesc) else "pinn_term_residual_system")
    _, cot = E._term_residual_sys(td, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True)
    calls = []
    for b, (c, key, nt, nx) in zip(td.blocks(), td.launches()):
        line = E._launch_line(key)
        who = f"field {eq.fields[c]}, {'direction' if isinstance(key, tuple) else 'axis'} {key}, set ({nt}, {nx})"
        calls.append((f"pinn_jet_forward, {who}", lambda c=c, nt=nt, nx=nx, line=line: E.jets_forward(prog, x, t, nt, nx, component=c, **line)))
        calls.append((f"pinn_jet_backward, {who}",
                      lambda c=c, b=b, nt=nt, nx=nx, line=line: E.jets_backward(prog, x, t, nt, nx, cot[b], flat, component=c, **line)))
    calls.append((f"{entry} (loss sum + cotangents, two launches)",
                  lambda: E._term_residual_sys(td, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True)))
    calls.append((f"{entry} (residuals only, one launch)", lambda: E._term_residual_sys(td, jets, x, t)))
    if isinstance(td, E.InvSystemTermDesc):  # the launch the step takes: with the parameter gradients
        pg = torch.zeros(int(td.desc.n_params), device=B.dev)
        calls.append((f"{entry} (loss sum + cotangents + param_grads, two launches)",
                      lambda: E._term_residual_sys(td, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True,
                                                   param_grads=pg)))
    if tag == "S4":  # the same program and blocks through the mixed entry point with all pair orders 0: the larger LDS footprint
        tm = E.MixedSystemTermDesc(td.terms, td.equation_of, td.coef_values, td.dimension, td.n_fields, td.n_equations, td.nt, td.nx, None,
                                   td.eq_weights)
        calls.append(("pinn_term_residual_system_mixed, all pair orders 0 (loss sum + cotangents, two launches)",
                      lambda: E.term_residual_system_mixed(tm, jets, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s, want_cotangents=True)))
        calls.append(("pinn_term_residual_system_mixed, all pair orders 0 (residuals only, one launch)",
                      lambda: E.term_residual_system_mixed(tm, jets, x, t)))
    if isinstance(td, E.FnSystemTermDesc) and not isinstance(td, E.NlSystemTermDesc):  # the kernel alone on values held, and the evaluation of the functions alone
        fv = td.fn_values(x, t)
        calls.append(("pinn_term_residual_system_fn on given values (loss sum + cotangents, two launches)",
                      lambda: E.term_residual_system_fn(td, jets, fv, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s,
                                                        want_cotangents=True)))
        calls.append(("fn_values: the functions' torch ops", lambda: td.fn_values(x, t)))
    if tag == "S3":  # the same program and blocks through the function entry point with no function named
        tf = E.FnSystemTermDesc(td.terms, td.equation_of, td.coef_values, td.dimension, td.n_fields, td.n_equations, td.nt, td.nx, td.pair,
                                (), td.eq_weights)
        calls.append(("pinn_term_residual_system_fn, no function named (loss sum + cotangents, two launches)",
                      lambda: E.term_residual_system_fn(tf, jets, None, x, t, grad_scale=1.0 / n, want_residual=False, loss_sum=s,
                                                        want_cotangents=True)))
        calls.append(("pinn_term_residual_system_fn, no function named (residuals only, one launch)",
                      lambda: E.term_residual_system_fn(tf, jets, None, x, t)))
    calls.append(("the chain through engine.residual_loss_grad", lambda: E.residual_loss_grad(prog, td, x, t, 1.0 / n, flat, loss_sum=s)))
    print()
    print(f"| {tag} launch ({n} points) | ms |")
    print("|---|---|")
    for label, fn in calls:
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"| {label} | {a.elapsed_time(b) / iters:.4f} |", flush=True)


def learned_values(tag, steps):
    """Train the inverse twin for `steps` captured steps (fresh samples, the default Adam) and print what it learned."""
    torch.manual_seed(0)
    name, net, eq, agent, cfg, n_req = build(tag)
    tr = PDETrainer(net, eq, None, cfg, device=B.dev, fast_step=False)
    tr._build_flat_state()
    start = eq.learned_values()
    replay, losses = tr.make_graphed_step(n_req)
    for _ in range(steps):
        replay()
    torch.cuda.synchronize()
    print()
    print(f"{tag} after {steps} captured steps (lr {cfg.training.learning_rate:g}): learned {eq.learned_values()} from {start}; "
          f"losses {({k: float(v) for k, v in losses.items()})}", flush=True)


def time_causal_launches(tag, causal, iters=20):
    """Device time of the launches of the causal chain, each on its own, and of the one fused launch they replace."""
    torch.manual_seed(0)
    name, net, eq, n_req = B.CONFIGS[tag]()
    if eq.dimension != 1:  # the chain (and t as one column of the batch) is the 1-D launch list's
        return
    x, t = eq.generate_collocation_points(n_req, strategy="uniform")
    prog, pd = net.program(), eq._pde_desc()
    loss, delta = eq._loss_function_name(), eq._huber_delta()
    n = int(x.shape[0])
    nt, nx = E.pde_streams(pd)
    flat, s = E.new_flat_grad(prog, B.dev), torch.zeros(1, device=B.dev)
    eps_dev = torch.tensor([causal[1]], dtype=torch.float32, device=B.dev)
    t_lo, t_hi = eq.time_domain
    r, _ = E.residual_forward(prog, pd, x, t, want_loss_sum=False)
    tt = t.reshape(-1).contiguous()
    cot, bl, bw = E.causal_weights(r.reshape(-1), tt, causal[0], t_lo, t_hi, eps_dev, loss, delta, 1.0 / n, loss_sum=s)
    scratch = torch.zeros(E._lib.PINN_CAUSAL_SCRATCH_DOUBLES, dtype=torch.float64, device=B.dev)
    calls = [("pinn_residual_forward (residual only)", lambda: E.residual_forward(prog, pd, x, t, want_loss_sum=False)),
             ("pinn_causal_weights (three launches)",
              lambda: E.causal_weights(r.reshape(-1), tt, causal[0], t_lo, t_hi, eps_dev, loss, delta, 1.0 / n, loss_sum=s, cot=cot,
                                       bin_losses=bl, bin_weights=bw, scratch=scratch)),
             ("pinn_residual_backward", lambda: E.residual_backward(prog, pd, x, t, cot, flat)),
             ("the one fused launch: pinn_residual_loss_grad", lambda: E.residual_loss_grad(prog, pd, x, t, 1.0 / n, flat, loss_sum=s))]
    print()
    print(f"| {tag} launch ({n} points, kernels {E._lib.kernel_name(prog, n, nt, nx, 0)} / {E._lib.kernel_name(prog, n, nt, nx, 1)}) | ms |")
    print("|---|---|")
    for label, fn in calls:
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"| {label} | {a.elapsed_time(b) / iters:.4f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,C3,C4")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--modes", default="autograd,manual,graph")
    ap.add_argument("--adaptive", choices=["none", "rbw", "lrw"], default="none")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--optimizer", choices=["adam", "lbfgs"], default="adam")
    ap.add_argument("--smoothness", type=float, default=0.0, help="C1 only: weight of HeatEquation's smoothness term")
    ap.add_argument("--term-pde", action="store_true", help="C2 only: Burgers as a TermPDE, and the chain's launches on their own")
    ap.add_argument("--causal", default="", metavar="M,EPS", help="causal residual weighting: M time bins, sharpness EPS")
    ap.add_argument("--term-nd", action="store_true", help="N1, N2: the heat Laplacian in 1-D (TermPDE) and 2-D (TermPDEnD), fourier 4x128")
    ap.add_argument("--term-mixed", action="store_true",
                    help="M1, M2, M3: 2-D heat (TermPDEnD), anisotropic diffusion and Cahn-Hilliard (TermPDEMixed), fourier 4x128")
    ap.add_argument("--system", choices=["gray_scott", "navier_stokes", "elasticity", "elasticity_nomixed", "navier_stokes_forced",
                                         "advection_diffusion", "euler_nl", "navier_stokes_inverse"], default=None,
                    help="N1, S1 (gray_scott) or N2, S2 (navier_stokes): a TermPDESystem beside the single-field step; S3 (elasticity): 2-D "
                         "elasticity as a TermPDESystemMixed; S4 (elasticity_nomixed): the same without its mixed terms; S2, S5 "
                         "(navier_stokes_forced): Navier-Stokes and its twin with a body force given as functions; S6 "
                         "(advection_diffusion): one field with a(x,y), b(x,y), kappa(x,y) as functions; S7, S8 (euler_nl): 1-D Euler in "
                         "(rho, u, p) with 1 / (2 + rho) as a nonlinear factor beside its twin without; S2, S9 (navier_stokes_inverse): "
                         "Navier-Stokes and its inverse twin with lam and nu learnable and velocity observations; fourier 4x128")
    ap.add_argument("--learned", type=int, default=0, metavar="STEPS",
                    help="S9 only: after the tables, train S9 for STEPS captured steps and print the learned values")
    args = ap.parse_args()
    if args.system and args.configs == "C1,C2,C3,C4":
        args.configs = {"gray_scott": "N1,S1", "navier_stokes": "N2,S2", "elasticity": "S3", "elasticity_nomixed": "S4",
                        "navier_stokes_forced": "S2,S5", "advection_diffusion": "S6", "euler_nl": "S7,S8",
                        "navier_stokes_inverse": "S2,S9"}[args.system]
    if args.term_nd and args.configs == "C1,C2,C3,C4":
        args.configs = "N1,N2"
    if args.term_mixed and args.configs == "C1,C2,C3,C4":
        args.configs = "M1,M2,M3"
    causal = None
    if args.causal:
        m, e = args.causal.split(",")
        causal = (int(m), float(e))
    if args.term_pde and args.configs == "C1,C2,C3,C4":
        args.configs = "C2"
    if args.optimizer == "lbfgs":
        return bench_lbfgs(args)
    print("| config | points | sampler | mode | ms/step | points/s | last total loss |")
    print("|---|---|---|---|---|---|---|")
    for tag in [c for c in args.configs.split(",") if c]:
        for mode in args.modes.split(","):
            if args.smoothness > 0 and tag != "C1":
                print(f"| {tag} | - | - | {mode} | not covered: --smoothness applies to C1 (HeatEquation) only | | |")
                continue
            if args.term_pde and tag != "C2":
                print(f"| {tag} | - | - | {mode} | not covered: --term-pde applies to C2 (Burgers) only | | |")
                continue
            torch.manual_seed(0)
            name, net, eq, agent, cfg, n_req = build(tag, args.adaptive, args.smoothness, args.term_pde, causal)
            tr = PDETrainer(net, eq, None, cfg, device=B.dev, rl_agent=agent, fast_step=False)
            if mode != "autograd":
                why = tr._manual_step_unsupported()
                if why is not None:
                    print(f"| {tag} | - | - | {mode} | not covered: {why} | | |")
                    continue
                tr._build_flat_state()
            if mode == "graph":
                run, losses = tr.make_graphed_step(n_req)
            else:
                def run(tr=tr, n_req=n_req):
                    x, t = tr._sample(n_req)
                    return tr.train_step(x, t)
                losses = run()
            n = int(tr._sample(n_req)[0].shape[0])
            for _ in range(3):
                out = run()
            times = []
            for _ in range(max(args.repeats, 1)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    out = run()
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0) / args.steps)
            ms = sorted(times)[len(times) // 2]
            spread = f" ({min(times):.3f}-{max(times):.3f})" if len(times) > 1 else ""
            last = losses if mode == "graph" else out
            sampler = "adaptive (DQN)" if agent is not None else cfg.training.collocation_distribution
            if args.adaptive != "none":
                mode = f"{mode} + {args.adaptive}"
            print(f"| {tag} {name} | {n} | {sampler} | {mode} | {ms:.3f}{spread} | {n / ms * 1e3:.3e} | {float(last['total'].detach()):.4e} |", flush=True)
            del tr, net, eq
            torch.cuda.empty_cache()
        if args.term_pde and tag == "C2":
            time_term_launches(tag)
        if args.term_mixed and tag in ND_CONFIGS:
            time_nd_launches(tag)
        if args.system and tag in ("S1", "S2", "S3", "S4", "S5", "S6", "S7", "S8", "S9"):
            time_system_launches(tag)
        if args.learned > 0 and tag == "S9":
            learned_values(tag, args.learned)
        if args.system and tag == "N2":
            time_nd_launches(tag)
        if causal is not None and not args.term_pde:
            time_causal_launches(tag, causal)


if __name__ == "__main__":
    main()
