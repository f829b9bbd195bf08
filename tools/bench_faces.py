"""Timings behind profiles/term_faces_step.md: the boundary chain of `TermPDEnD` with per-face conditions.

  python tools/bench_faces.py step              launch-list step time (eager and captured) of the README's 2-D and 3-D heat
                                                problems, default point counts, 5 000 collocation points, fourier 4 x 128, in
                                                three forms: the config Dirichlet form, the same conditions through
                                                face_conditions, all faces Neumann.  The forms alternate window by window.
  python tools/bench_faces.py kernels 2|3       the loss-term calls alone on that problem's fixed points, Dirichlet on every face +
                                                the initial term: pinn_jet_losses (2 terms) and pinn_face_losses (2 dim + 1
                                                terms), 200 calls each — run under `rocprofv3 --kernel-trace --stats` and
                                                read the per-kernel averages with tools/kstats.py.
"""

import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PI = torch.pi
D0 = {"type": "dirichlet", "value": 0.0}
N0 = {"type": "neumann", "value": 0.0}
FORMS = {"config dirichlet": (None, {"dirichlet": {"type": "fixed", "value": 0.0}}), "faces dirichlet": ({"default": D0}, {}),
         "faces neumann": ({"default": N0}, {})}


def build(dim, form, dev):
    from pinnrl_amd import pdes as P
    from pinnrl_amd.config import Config, ModelConfig, TrainingConfig
    from pinnrl_amd.neural_networks import PINNModel
    from pinnrl_amd.training import PDETrainer

    faces, bcs = FORMS[form]
    cfg = Config.__new__(Config)
    cfg.device = dev
    cfg.training = TrainingConfig(learning_rate=1e-3, gradient_clipping=1.0, optimizer="adam")
    cfg.model = ModelConfig(input_dim=dim + 1, hidden_dim=128, output_dim=1, num_layers=4, activation="tanh", architecture="fourier")
    cfg.model.mapping_size, cfg.model.scale = 64, 1.0
    torch.manual_seed(0)
    model = PINNModel(cfg, device=dev)
    pc = P.PDEConfig(name=f"heat {dim}D", domain=[(0.0, 1.0)] * dim, time_domain=(0.0, 1.0), parameters={"alpha": 0.05},
                     boundary_conditions=dict(bcs), initial_condition={}, exact_solution={}, dimension=dim, device=dev, training=cfg.training)
    terms = [(1.0, ("u_t",))] + [((-1.0, "alpha"), (f"u_{ax}{ax}",)) for ax in "xyz"[:dim]]
    fn = torch.sin if faces is None or faces["default"] is D0 else torch.cos
    pde = P.TermPDEnD(pc, terms, lambda x: torch.prod(fn(PI * x), dim=1), face_conditions=faces)
    tr = PDETrainer(model, pde, {}, cfg, device=dev)
    assert tr._manual_step_unsupported() is None, tr._manual_step_unsupported()
    tr._build_flat_state()
    return tr, pde


def step_times(dev, n_batch=5000, windows=7, steps=100):
    out = {}
    for dim in (2, 3):
        runs = {}
        for form in FORMS:
            tr, pde = build(dim, form, dev)
            torch.manual_seed(1)
            xb, tb = pde._sample_uniform(n_batch)
            for _ in range(30):
                tr.train_step(xb, tb)
            tr._sample = lambda n, xb=xb, tb=tb: (xb, tb)
            replay, _ = tr.make_graphed_step(n_batch, warmup=2)
            for _ in range(30):
                replay()
            runs[form] = (lambda tr=tr, xb=xb, tb=tb: tr._manual_launches(xb, tb), replay)
        times = {form: ([], []) for form in FORMS}
        for _ in range(windows):  # the forms alternate: a drift of the machine lands on all of them
            for form, fns in runs.items():
                for k, fn in enumerate(fns):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fn()
                    torch.cuda.synchronize()
                    times[form][k].append((time.perf_counter() - t0) / steps * 1e3)
        for form, (eager, graph) in times.items():
            out[f"{dim}D {form}"] = {"eager_ms": statistics.median(eager), "eager_min_max": [min(eager), max(eager)],
                                      "captured_ms": statistics.median(graph), "captured_min_max": [min(graph), max(graph)]}
            print(f"{dim}-D {form:18s} eager {statistics.median(eager):.3f} ms [{min(eager):.3f}, {max(eager):.3f}]   "
                  f"captured {statistics.median(graph):.3f} ms [{min(graph):.3f}, {max(graph):.3f}]", flush=True)
    return out


def loss_calls(dev, dim, calls=200):
    from pinnrl_amd import _lib
    from pinnrl_amd import engine as E
    from pinnrl_amd.pdes.term_pde_nd import box_points

    P = box_points([(0.0, 1.0)] * dim, (0.0, 1.0), dim, 16, 32, dev)
    nf, nbc, nic = P["n_face"], P["n_bc"], P["n_ic"]
    n = nbc + nic
    torch.manual_seed(0)
    u = torch.randn(1, n, device=dev)
    ub, u0 = torch.zeros(nbc, device=dev), torch.randn(nic, device=dev)
    tl, cot = torch.zeros(8, device=dev), torch.zeros(1, n, device=dev)
    old = [(0, nbc, 0, 0, ub, 10.0), (nbc, n, 0, 0, u0, 10.0)]
    new = E.FaceTerms([{"n": nf, "alpha": 1.0, "value": k * nf, "target": 0.0, "weight": 10.0} for k in range(2 * dim)]
                      + [{"n": nic, "alpha": 1.0, "value": nbc, "target": u0, "weight": 10.0}])
    tl2, cot2 = torch.zeros(32, device=dev), torch.zeros(n, device=dev)
    scratch = torch.zeros(_lib.PINN_FACE_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    s4, rs = torch.zeros(4, device=dev), torch.ones(1, device=dev)
    for _ in range(calls):
        E.jet_losses(u, old, "mse", 1.0, tl, cot, residual_sum=rs, residual_scale=1.0, residual_weight=1.0, n_boundary_terms=1, summary4=s4)
        E.face_losses(u.reshape(-1), new, "mse", 1.0, tl2, cot2, scratch, residual_sum=rs, residual_scale=1.0, residual_weight=1.0,
                      n_boundary_terms=2 * dim, summary4=s4)
    torch.cuda.synchronize()
    # same losses (one mean over all faces against 2 dim means of equal length) and the same cotangents up to the grouping
    assert abs(float(tl[0]) - float(tl2[: 2 * dim].mean())) <= 1e-5 * abs(float(tl[0])) and abs(float(tl[1]) - float(tl2[2 * dim])) <= 1e-6
    print(f"{dim}-D: {n} fixed points ({nbc} boundary + {nic} initial), {calls} calls of each entry point")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "measurements need the GPU"
    dev = torch.device("cuda:0")
    if sys.argv[1] == "step":
        print(json.dumps(step_times(dev)))  # the table again, as one JSON line
    else:
        loss_calls(dev, int(sys.argv[2]))
