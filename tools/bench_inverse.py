"""Inverse problems (trainable Burgers nu) on the headline network, fourier 4x128: cost of the residual launch and of the
whole training step (events on the launch stream, warm-up, median of --reps; requires a GPU, no fallback).

    python tools/bench_inverse.py [--reps 20] [--rounds 3] [--skip-steps] [--points 49729 4900]

Residual launch, N = 49 729 and 4 900, variants alternated over --rounds rounds (spread = (max - min) / median of the
per-round medians):
  inverse        pinn_residual_loss_grad_inverse: nu read from a device array, d/d nu from the same launch
  by_value       pinn_residual_loss_grad with the same nu by value (no coefficient gradient)
  coef_lm        pinn_residual_loss_grad_coef with PINN_FLAG_LAYER_MAJOR (how inverse mode ran before the COEF units)
Training step, inverse mode with 200 observations, batch 49 729 and 4 900:
  autograd       compute_loss -> backward -> clip -> torch Adam
  launch_list    PDETrainer's autograd-free launch list (eager)
  graph          the same captured in a graph and replayed
Prints one JSON line per measurement group.
"""

import argparse
import copy
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def _summary(per_round):
    med = statistics.median(per_round)
    return {"ms": round(med, 4), "spread": round((max(per_round) - min(per_round)) / med, 4), "rounds": [round(v, 4) for v in per_round]}


def _setup(dev, inverse=True):
    import pinnrl_amd  # noqa: F401
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel
    from pinnrl_amd.pdes import BurgersEquation, PDEConfig

    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.model = ModelConfig(input_dim=2, hidden_dim=128, output_dim=1, num_layers=4, activation="tanh", architecture="fourier")
    cfg.model.mapping_size, cfg.model.scale = 32, 10.0
    torch.manual_seed(0)
    model = PINNModel(cfg, device=dev)
    tr = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, mode="inverse" if inverse else "forward")
    cfg.training = tr
    pde = BurgersEquation(PDEConfig(
        name="burgers", domain=[(-1.0, 1.0)], time_domain=(0.0, 1.0), parameters={"nu": 0.01 / math.pi},
        boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0}, exact_solution={}, dimension=1, device=dev,
        training=tr, trainable_parameters=["nu"] if inverse else [], parameter_initial_guesses={"nu": 0.05} if inverse else {}))
    if inverse:
        g = torch.Generator().manual_seed(3)
        xo, to = torch.rand(200, 1, generator=g) * 2 - 1, torch.rand(200, 1, generator=g)
        pde.observation_data = {"x": xo.to(dev), "t": to.to(dev), "u": (-torch.sin(math.pi * xo) * torch.exp(-to)).to(dev)}
    return cfg, model, pde


def bench_launch(dev, N, reps, rounds):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    cfg, model, pde = _setup(dev)
    prog = model.program()
    lm = copy.copy(prog)
    lm.desc = copy.copy(prog.desc)
    lm.desc.flags |= _lib.PINN_FLAG_LAYER_MAJOR
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(N, 1, device=dev, generator=g) * 2 - 1
    t = torch.rand(N, 1, device=dev, generator=g)
    nu = 0.05
    pd = E.pde_desc("burgers", 1, [nu])
    cv = torch.tensor([nu, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    flat = E.new_flat_grad(prog, dev)
    cg = torch.zeros(4, dtype=torch.float32, device=dev)
    s = torch.zeros(1, dtype=torch.float32, device=dev)
    legs = {
        "inverse": lambda: E.residual_loss_grad_inverse(prog, pd, cv, x, t, 1.0 / N, flat, cg, loss_sum=s),
        "by_value": lambda: E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat, loss_sum=s),
        "coef_lm": lambda: E.residual_loss_grad(lm, pd, x, t, 1.0 / N, flat, loss_sum=s, coef_grads=cg),
    }
    per = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            per[k].append(_time(fn, reps))
    row = {"what": "residual_launch", "N": N, "kernel": E.inverse_kernel_name(prog, pd, N)}
    row.update({k: _summary(v) for k, v in per.items()})
    row["inverse_vs_by_value"] = round(row["inverse"]["ms"] / row["by_value"]["ms"], 4)
    row["coef_lm_vs_inverse"] = round(row["coef_lm"]["ms"] / row["inverse"]["ms"], 4)
    print(json.dumps(row), flush=True)


def bench_step(dev, N, reps, rounds):
    from pinnrl_amd.training import PDETrainer

    trainers = {}
    for leg in ("autograd", "launch_list", "graph"):
        cfg, model, pde = _setup(dev)
        tr = PDETrainer(model, pde, {}, cfg, device=dev, fast_step=False if leg == "autograd" else None)
        torch.manual_seed(0)
        xb, tb = pde.generate_collocation_points(N, strategy="uniform")
        xb, tb = xb.to(dev), tb.to(dev)
        tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
        if leg == "autograd":
            fn = lambda tr=tr, xb=xb, tb=tb: tr.train_step(xb, tb)  # noqa: E731
        elif leg == "launch_list":
            why = tr._manual_step_unsupported()
            if why is not None:
                raise RuntimeError(f"launch list does not cover the inverse configuration: {why}")
            tr._build_flat_state()
            fn = lambda tr=tr, xb=xb, tb=tb: tr.train_step(xb, tb)  # noqa: E731
        else:
            fn, _ = tr.make_graphed_step(N, warmup=2)
        trainers[leg] = (tr, fn)
    per = {k: [] for k in trainers}
    for _ in range(rounds):
        for k, (_, fn) in trainers.items():
            per[k].append(_time(fn, reps))
    row = {"what": "inverse_training_step", "N": N}
    row.update({k: _summary(v) for k, v in per.items()})
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--points", type=int, nargs="+", default=[49729, 4900])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_inverse.py needs a ROCm device")
    dev = torch.device("cuda:0")
    for N in args.points:
        bench_launch(dev, N, args.reps, args.rounds)
    if not args.skip_steps:
        for N in args.points:
            bench_step(dev, N, args.reps, args.rounds)


if __name__ == "__main__":
    main()
