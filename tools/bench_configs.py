"""Residual+grad throughput of the five BASELINE.json configurations on ONE GPU (context for DESIGN.md §8).

    python tools/bench_configs.py [--steps 10] [--only C3,C4] [--rounds 3]

C2 is the headline (bench.py); the others are parity-test configurations timed here for information:
one fused `pinn_residual_loss_grad` launch per step, points and weights resident.  C6 is the autoencoder of the
reference's shipped config.yaml and C6y its yardstick, the feedforward + LayerNorm network with the same GEMMs (plus a
LayerNorm and an activation on the 64-wide layer).  --rounds R times the selected configurations R times in alternation
(C6, C6y, C6, C6y, ...) and adds one line per configuration with the median and the spread over the rounds.
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import pinnrl_amd  # noqa: E402,F401
from pinnrl_amd import engine as E  # noqa: E402
from pinnrl_amd import pdes as P  # noqa: E402
from pinnrl_amd.config import Config, ModelConfig  # noqa: E402
from pinnrl_amd.neural_networks import PINNModel  # noqa: E402

dev = torch.device("cuda:0")


def model(arch, hidden, layers, act, input_dim=2, **extra):
    cfg = Config.__new__(Config)
    cfg.device = torch.device("cpu")
    cfg.model = ModelConfig(input_dim=input_dim, hidden_dim=hidden, output_dim=1, num_layers=layers, activation=act,
                            architecture=arch)
    for k, v in extra.items():
        setattr(cfg.model, k, v)
    torch.manual_seed(0)
    return PINNModel(cfg, device=torch.device("cpu")).to(dev)


def pde(cls, domain, tdom, params, ic, dimension=1):
    return cls(P.PDEConfig(name=cls.__name__, domain=domain, time_domain=tdom, parameters=params,
                           boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}}, initial_condition=ic,
                           exact_solution={}, dimension=dimension, device=dev))


CONFIGS = {
    "C1": lambda: ("Heat 1D a=0.01, fourier 4x128", model("fourier", 128, 4, "tanh"),
                   pde(P.HeatEquation, [(0.0, 1.0)], (0.0, 1.0), {"alpha": 0.01}, {"type": "sine"}), 5000),
    "C2": lambda: ("Burgers 1D nu=0.01/pi, fourier 4x128", model("fourier", 128, 4, "tanh"),
                   pde(P.BurgersEquation, [(-1.0, 1.0)], (0.0, 1.0), {"nu": 0.01 / math.pi}, {"type": "sine"}), 50000),
    "C3": lambda: ("Allen-Cahn 1D eps=0.01, resnet 6x256", model("resnet", 256, 6, "tanh", num_blocks=6),
                   pde(P.AllenCahnEquation, [(-1.0, 1.0)], (0.0, 1.0), {"epsilon": 0.01}, {"type": "tanh"}), 100000),
    "C4": lambda: ("KdV 1D, siren w0=30 8x256", model("siren", 256, 8, "tanh", omega_0=30.0),
                   pde(P.KdVEquation, [(-15.0, 15.0)], (0.0, 5.0), {"speed": 1.0}, {"type": "soliton"}), 200000),
    "C5": lambda: ("Cahn-Hilliard 2D, attention 4 layers x128 (4 heads)", model("attention", 128, 4, "gelu", input_dim=3, num_heads=4),
                   pde(P.CahnHilliardEquation, [(0.0, 1.0), (0.0, 1.0)], (0.0, 1.0), {"epsilon": 0.01}, {"type": "tanh"}, 2), 1000000),
    "C6": lambda: ("Burgers 1D nu=0.01/pi, autoencoder [124, 248, 124] latent 64, relu + LayerNorm",
                   model("autoencoder", 124, 3, "relu", hidden_dims=[124, 248, 124], latent_dim=64, layer_norm=True),
                   pde(P.BurgersEquation, [(-1.0, 1.0)], (0.0, 1.0), {"nu": 0.01 / math.pi}, {"type": "sine"}), 50000),
    "C6y": lambda: ("Burgers 1D nu=0.01/pi, feedforward [124, 248, 124, 64, 124, 248, 124], relu + LayerNorm",
                    model("feedforward", 124, 7, "relu", hidden_dims=[124, 248, 124, 64, 124, 248, 124], layer_norm=True),
                    pde(P.BurgersEquation, [(-1.0, 1.0)], (0.0, 1.0), {"nu": 0.01 / math.pi}, {"type": "sine"}), 50000),
}


def prepare(tag):
    name, net, eq, n_req = CONFIGS[tag]()
    torch.manual_seed(1)
    if tag == "C3":  # adaptive sampling yields exactly N points; throughput is distribution-independent
        x = torch.rand(n_req, 1, device=dev) * 2 - 1
        t = torch.rand(n_req, 1, device=dev)
    else:
        x, t = eq.generate_collocation_points(n_req, strategy="uniform")
    prog, pd = net.program(), eq._pde_desc()
    return name, net, prog, pd, x, t, E.new_flat_grad(prog, dev)


def time_one(tag, ready, steps):
    name, net, prog, pd, x, t, flat = ready
    N = x.shape[0]
    nt, nx = E.pde_streams(pd)
    K = 1 + nt + nx
    for _ in range(3):
        flat.zero_()
        E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        flat.zero_()
        E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    tf = 3 * K * prog.flops_per_point() * N / (ms * 1e-3) / 1e12
    print(f"| {tag} {name} | {N} | {net.count_parameters()} | {K} | {ms:.3f} | {N / ms * 1e3:.3e} | {tf:.1f} | {tf / 157.3:.3f} |", flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    only = [s for s in args.only.split(",") if s]
    tags = [tag for tag in CONFIGS if not only or tag in only]
    print("| config | points | params | K | ms/step | points/s | TFLOP/s (3 K F_fwd) | frac of 157.3 |")
    print("|---|---|---|---|---|---|---|---|")
    if args.rounds <= 1:  # one configuration resident at a time
        for tag in tags:
            time_one(tag, prepare(tag), args.steps)
        return
    ready = {tag: prepare(tag) for tag in tags}  # alternation needs the selected configurations resident together
    times = {tag: [] for tag in tags}
    for _ in range(args.rounds):
        for tag in tags:
            times[tag].append(time_one(tag, ready[tag], args.steps))
    for tag, ms in times.items():
        s = sorted(ms)
        print(f"{tag}: median {s[len(s) // 2]:.3f} ms over {len(s)} rounds, min {s[0]:.3f}, max {s[-1]:.3f} "
              f"(spread {100 * (s[-1] - s[0]) / s[len(s) // 2]:.1f} % of the median)", flush=True)


if __name__ == "__main__":
    main()
