"""Cost of input cotangents: pinn_jet_backward vs pinn_jet_backward_inputs on the same problem (events on the launch stream).

    python tools/bench_input_grad.py [--reps 20]

Legs per configuration (median ms of --reps timed calls after warm-up):
  jet_backward          pinn_jet_backward as the descriptor routes it (fourier 4x128: the fused tile-major kernel)
  jet_backward_lm       pinn_jet_backward on the layer-major engine (PINN_FLAG_LAYER_MAJOR, a private descriptor copy)
  inputs+weights        pinn_jet_backward_inputs with weight gradients and x_grad / t_grad
  inputs_only           pinn_jet_backward_inputs without a weight-gradient table
Prints one JSON line per configuration.
"""

import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _model(arch, dev):
    import oracle as O
    import pinnrl_amd  # noqa: F401
    from pinnrl_amd.config import Config, ModelConfig
    from pinnrl_amd.neural_networks import PINNModel

    spec = O.ArchSpec(architecture=arch, input_dim=2, hidden_dim=128, num_layers=4, num_heads=4, activation="tanh")
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.model = ModelConfig(input_dim=2, hidden_dim=128, output_dim=1, num_layers=4, activation="tanh", architecture=arch)
    cfg.model.mapping_size, cfg.model.scale, cfg.model.num_heads = spec.mapping_size, spec.scale, spec.num_heads
    torch.manual_seed(0)
    return PINNModel(cfg, device=dev)


def _time(fn, reps):
    for _ in range(3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E

    dev = torch.device("cuda:0")
    for arch, N, orders in (("fourier", 49729, [(0, 0), (1, 2)]), ("attention", 10 ** 6, [(1, 2)])):
        model = _model(arch, dev)
        prog = model.program()
        lm = copy.copy(prog)
        lm.desc = copy.copy(prog.desc)
        lm.desc.flags |= _lib.PINN_FLAG_LAYER_MAJOR
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand(N, 1, device=dev, generator=g) * 2 - 1
        t = torch.rand(N, 1, device=dev, generator=g)
        for nt, nx in orders:
            cot = torch.randn(1 + nt + nx, N, device=dev, generator=g)
            flat = E.new_flat_grad(prog, dev)
            row = {"arch": arch, "width": 128, "layers": 4, "N": N, "orders": [nt, nx]}
            row["jet_backward_ms"] = _time(lambda: E.jets_backward(prog, x, t, nt, nx, cot, flat), args.reps)
            row["jet_backward_lm_ms"] = _time(lambda: E.jets_backward(lm, x, t, nt, nx, cot, flat), args.reps)
            row["inputs+weights_ms"] = _time(lambda: E.jets_backward_inputs(prog, x, t, nt, nx, cot, flat, True, True), args.reps)
            row["inputs_only_ms"] = _time(lambda: E.jets_backward_inputs(prog, x, t, nt, nx, cot, None, True, True), args.reps)
            row["overhead_vs_lm"] = round(row["inputs+weights_ms"] / row["jet_backward_lm_ms"] - 1.0, 4)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
