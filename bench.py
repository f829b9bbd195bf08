"""Headline benchmark: collocation-points/sec of one residual+grad evaluation + final residual L2, Burgers 1D
(BASELINE.json `metric`, configs[1]).

A "step" = zero the gradient buffer, then ONE fused launch that computes r = compute_residual(model, x, t), sum r^2
and d(mean r^2)/d(theta) for this rank's collocation points (weights and points resident in HBM), then — with more
than one rank — one RCCL all-reduce of [flat gradient || loss sum].

    python bench.py --gpus 1 --steps 50 --warmup 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W [--scaling strong --points 1000000]

--scaling weak (default): every rank owns its own 49 729-point batch.  --scaling strong: ONE global batch of --points
points (north_star: ">= 6x strong scaling at 8 GPUs"), sampled identically on every rank and split by
`pinnrl_amd.distributed.shard_bounds`; `value` is then global points/s.

A plain run sets up, warms up, times --steps steps and prints the result line (+ --dump-outputs).  With --full the
line also carries (all outside the timed region): the sustained-clock figure, and for N = 1 the CPU oracle on the same
points (`cpu_baseline`, all host threads and one thread), the 4 900-point figure north_star quotes its >= 10x target
on, the second half of the metric — `training.final_residual_l2` after a fixed 200-step Adam schedule on the GPU and
on the CPU from identical theta_0 and batches — and the per-kernel figures of the other BASELINE configurations; for
N > 1 the 10^6-point strong-scaling figure and BASELINE configs[3]/[4] in their sharded form.

--dump-outputs DIR writes what the last timed step computed, as a caller of the step receives it: DIR/grad.npy (the
gradient of the trainable tensors in parameter order, float32, 41 473 values) and DIR/loss_sum.npy (sum of r^2 over the points, float32).  Inputs (theta_0,
collocation points) are seeded, so two builds run with the same arguments can be compared output for output.
"""

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense


def pmc_traffic():
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of THIS command
    (profiles/r02_bench.json, made by tools/profile_summary.py): FETCH_SIZE (x2: gfx950 counts 64 B per 128-B
    request) + WRITE_SIZE, both KiB.  None when no profile has been committed."""
    for name in ("r03_bench.json", "r02_bench.json", "r01_bench.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                h = json.load(f).get("hbm_bytes_per_launch")
            if h:
                return float(h["read_x2"] + h["write"]), "profiles/" + name
        except (OSError, ValueError, KeyError):
            continue
    return None, None


def host_threads() -> int:
    """Threads for the CPU leg: this process's CPU share (a 1-GPU box grants 16 cores), never the whole host."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("PINN_CPU_THREADS", "16"))))


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_eval(O, pspec, aspec, sd, x_cpu, t_cpu, seconds, threads):
    """Best-of timing of the oracle (= the reference's CPU op sequence: 2 forwards + chained autograd.grad + backward)."""
    torch.set_num_threads(threads)
    for _ in range(2):
        r, L, g = O.residual_loss_and_grad(pspec, aspec, sd, x_cpu, t_cpu)
    best, n, t_end = float("inf"), 0, time.perf_counter() + seconds
    while time.perf_counter() < t_end or n < 3:
        t0 = time.perf_counter()
        r, L, g = O.residual_loss_and_grad(pspec, aspec, sd, x_cpu, t_cpu)
        best = min(best, time.perf_counter() - t0)
        n += 1
    return x_cpu.shape[0] / best, n, float(L), g


def gpu_points_per_s(E, prog, pd, x, t, buf, n_grad, steps=30):
    flat, loss_sum = buf[:n_grad], buf[n_grad : n_grad + 1]
    for _ in range(5):
        buf.zero_()
        E.residual_loss_grad(prog, pd, x, t, 1.0 / x.shape[0], flat, loss_sum=loss_sum)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        buf.zero_()
        E.residual_loss_grad(prog, pd, x, t, 1.0 / x.shape[0], flat, loss_sum=loss_sum)
    torch.cuda.synchronize()
    return x.shape[0] * steps / (time.perf_counter() - t0)


def training_parity(dev, O, pspec, aspec, steps=200, batch=5000, lr=1e-3, clip=1.0):
    """Second half of the metric: sqrt(mean r^2) on the fixed 49 729-point grid after a fixed schedule, on the GPU
    (PDETrainer's autograd-free step) and on the CPU (oracle.compute_loss_terms + torch Adam + clip_grad_norm_) from
    the same theta_0 (seed 0) and the same batches (product sampler on the device, seed 2, copied to the host).

    Two controls put the 200-step theta distance into context: the SAME CPU schedule run with one thread
    instead of all of them (different fp32 summation orders inside the reference's own kernels), and a GPU run with
    deterministic reductions.  `theta_rel_l2_by_step` of each is the relative L2 distance to the all-threads CPU run."""
    from __graft_entry__ import _burgers
    from pinnrl_amd.config import TrainingConfig
    from pinnrl_amd.training import PDETrainer

    marks = (1, 3, 10, 30, 100, steps)

    def gpu_run(deterministic, batches=None):
        cfg, model, pde = _burgers(dev, hidden=128, layers=4, mapping=32, scale=10.0, seed=0)
        cfg.device = dev
        cfg.training = TrainingConfig(learning_rate=lr, gradient_clipping=clip)
        if deterministic:
            model.set_deterministic(True)
        tr = PDETrainer(model, pde, {}, cfg, device=dev)
        sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        assert tr._manual_step_unsupported() is None
        tr._build_flat_state()
        made, snaps = [], {}
        torch.manual_seed(2)
        for s in range(1, steps + 1):
            if batches is None:
                x, t = pde.generate_collocation_points(batch, strategy="uniform")
                made.append((x.cpu(), t.cpu()))
            else:
                x, t = batches[s - 1][0].to(dev), batches[s - 1][1].to(dev)
            tr.train_step(x, t)
            if s in marks:
                snaps[s] = torch.cat([p.detach().flatten().cpu() for _, p in model.named_parameters()])
        return model, pde, sd0, (made if batches is None else batches), snaps

    model, pde, sd0, batches, snaps = gpu_run(False)
    torch.manual_seed(3)
    xg, tg = pde.generate_collocation_points(50000, strategy="uniform")  # the fixed evaluation grid (49 729 points)
    with torch.no_grad():
        r_gpu = pde.compute_residual(model, xg, tg)
        u_gpu = model(torch.cat([xg, tg], 1))
    torch.cuda.synchronize()
    _, _, _, _, snaps_det = gpu_run(True, batches)
    torch.cuda.synchronize()

    bc = O.PdeSpec(name="burgers", parameters=pspec.parameters, boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
                   initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0})

    def cpu_run(threads, perturb=0.0):
        torch.set_num_threads(threads)
        params = {k: v.clone() for k, v in sd0.items()}
        if perturb:  # theta_0 (1 + perturb * N(0, 1)), fixed seed: one rounding error's worth of difference at step 0
            g = torch.Generator().manual_seed(9)
            params = {k: (v * (1.0 + perturb * torch.randn(v.shape, generator=g)) if k != "model.fourier.B" else v) for k, v in params.items()}
        params = {k: v.requires_grad_(k != "model.fourier.B") for k, v in params.items()}
        names = [k for k in params if params[k].requires_grad]
        opt = torch.optim.Adam([params[k] for k in names], lr=lr)
        out, t0 = {}, time.perf_counter()
        for s, (xb, tb) in enumerate(batches, start=1):
            opt.zero_grad()
            O.compute_loss_terms(bc, lambda z: O.network_forward(aspec, params, z), xb, tb)["total"].backward()
            torch.nn.utils.clip_grad_norm_([params[k] for k in names], clip)
            opt.step()
            if s in marks:
                out[s] = torch.cat([params[k].detach().flatten() for k in names])
        return params, out, time.perf_counter() - t0

    nthr = host_threads()
    params, ref, cpu_s = cpu_run(nthr)
    _, ref1, cpu1_s = cpu_run(1)
    _, refp, _ = cpu_run(nthr, perturb=1e-7)
    torch.set_num_threads(nthr)

    def drift(a):
        return {str(k): float((a[k] - ref[k]).norm() / ref[k].norm()) for k in sorted(ref)}

    def within(d):
        return max([int(k) for k, v in d.items() if v <= 1e-5], default=0)

    d_gpu, d_det, d_cpu1, d_cpup = drift(snaps), drift(snaps_det), drift(ref1), drift(refp)
    xc, tc = xg.cpu(), tg.cpu()
    sdT = {k: v.detach() for k, v in params.items()}
    r_cpu = O.compute_residual(pspec, lambda z: O.network_forward(aspec, sdT, z), xc, tc).detach()
    u_cpu = O.network_forward(aspec, sdT, torch.cat([xc, tc], 1)).detach()
    l2_gpu, l2_cpu = float(r_gpu.double().pow(2).mean().sqrt()), float(r_cpu.double().pow(2).mean().sqrt())
    return {
        "schedule": f"{steps} Adam steps (lr {lr}, clip {clip}, loss weights 1/10/10), {batches[0][0].shape[0]}-point batches from "
                    "pde.generate_collocation_points on the device (seed 2), theta_0 seed 0; GPU: PDETrainer autograd-free step, "
                    "CPU: oracle.compute_loss_terms + torch.optim.Adam",
        "final_residual_l2": l2_gpu, "final_residual_l2_cpu": l2_cpu,
        "final_residual_l2_rel_diff": abs(l2_gpu - l2_cpu) / l2_cpu,
        "residual_field_rel_l2": float((r_gpu.cpu() - r_cpu).norm() / r_cpu.norm()),
        "u_rel_l2": float((u_gpu.cpu() - u_cpu).norm() / u_cpu.norm()),
        "theta_rel_l2_by_step": d_gpu, "steps_within_1e-5": within(d_gpu),
        "gpu_deterministic": {"theta_rel_l2_by_step": d_det, "steps_within_1e-5": within(d_det),
                              "note": "same batches, PINNModel.set_deterministic(True): fixed-order gradient reductions (the "
                                      "store flush of the fused kernel reduces in a fixed order in the default mode too)"},
        "cpu_control": {"theta_rel_l2_by_step": d_cpu1, "steps_within_1e-5": within(d_cpu1), "threads": [nthr, 1],
                        "cpu_seconds_1thread": cpu1_s,
                        "note": "the reference CPU path against ITSELF: same schedule, same batches, 1 thread vs all threads "
                                "(summation order inside torch's CPU kernels) - the reference's own reproducibility envelope"},
        "cpu_perturbed": {"theta_rel_l2_by_step": d_cpup, "steps_within_1e-5": within(d_cpup), "relative_perturbation": 1e-7,
                          "note": "the reference CPU path against ITSELF from theta_0 (1 + 1e-7 N(0,1)): how fast this schedule amplifies "
                                  "a difference of one fp32 rounding error (machine-independent, unlike the thread-count control)"},
        "eval_grid_points": int(xg.shape[0]), "cpu_seconds": cpu_s,
    }


def secondary_configs(E):
    """Residual+grad of the other BASELINE configurations (parity-test cases, one GPU), for the record: engine, ms per
    step, fraction of the 157.3 TFLOP/s fp32 MFMA peak at 3 K F_fwd FLOP per point."""
    import bench_configs as B

    out = {}
    for tag in ("C1", "C3", "C4", "C5"):
        name, net, eq, n_req = B.CONFIGS[tag]()
        torch.manual_seed(1)
        sampler = "uniform"
        if tag == "C3":  # BASELINE C3: DQN adaptive sampling (pde_base.py:961-1073), exploit branch (spread over the domain)
            from pinnrl_amd.rl import RLAgent

            eq.rl_agent = RLAgent(state_dim=2, action_dim=1, hidden_dim=64, device=B.dev)
            eq.rl_agent.epsilon = 0.0
            x, t = eq.generate_collocation_points(n_req, strategy="adaptive")
            sampler = "adaptive (DQN agent, epsilon 0)"
        else:
            x, t = eq.generate_collocation_points(n_req, strategy="uniform")
        N = x.shape[0]
        prog, pd = net.program(), eq._pde_desc()
        nt, nx = E.pde_streams(pd)
        K = 1 + nt + nx
        flat = E.new_flat_grad(prog, B.dev)
        for _ in range(2):
            flat.zero_()
            E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat)
        torch.cuda.synchronize()
        steps = 3
        t0 = time.perf_counter()
        for _ in range(steps):
            flat.zero_()
            E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        tf = 3 * K * prog.flops_per_point() * N / (ms * 1e-3) / 1e12
        out[tag] = {"workload": name, "points": N, "sampler": sampler, "streams": K, "ms_per_step": ms, "points_per_s": N / ms * 1e3,
                    "tflops": tf, "frac": tf / PEAK_F32_MFMA_TFLOPS,
                    "engine": "fused tile-major kernel (jet_kernel_wide)" if tag == "C1" else
                              "layer-major engine (lm_fused / lm_gemm_nt8 / lm_gemm / lm_ew_*; per-kernel split: profiles/r03_" + tag + ".md)"}
        del net, eq, x, t, flat
        torch.cuda.empty_cache()
    return out


def sharded_configs(E, D, dist, dev, rank, world):
    """N > 1 only.  BASELINE configs[3] (KdV, siren 8x256, 200k points, "4xMI355X data-parallel") and configs[4]
    (Cahn-Hilliard 2-D, attention, 1M points "sharded 8xMI355X with RCCL loss all-reduce") in their multi-GPU form: ONE
    global batch (identical on every rank under a seed), contiguous row shards (distributed.shard_bounds), the local
    residual sum scaled by the GLOBAL 1/N, one in-place all-reduce of the flat gradient per step.  Max over ranks."""
    import bench_configs as B

    B.dev = dev
    out = {}
    for tag in ("C4", "C5"):
        name, net, eq, n_req = B.CONFIGS[tag]()  # theta_0 under a fixed seed: identical replicas
        torch.manual_seed(11)
        x, t = eq.generate_collocation_points(n_req, strategy="uniform")
        N = x.shape[0]
        lo, hi = D.shard_bounds(N, rank, world)
        xs, ts_ = x[lo:hi].contiguous(), t[lo:hi].contiguous()
        del x, t
        prog, pd = net.program(), eq._pde_desc()
        flat = E.new_flat_grad(prog, dev)
        for _ in range(2):
            flat.zero_()
            E.residual_loss_grad(prog, pd, xs, ts_, 1.0 / N, flat)
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        torch.cuda.synchronize()
        dist.barrier()
        steps = 5
        t0 = time.perf_counter()
        for _ in range(steps):
            flat.zero_()
            E.residual_loss_grad(prog, pd, xs, ts_, 1.0 / N, flat)
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        torch.cuda.synchronize()
        ms = torch.tensor([1e3 * (time.perf_counter() - t0) / steps], dtype=torch.float64, device=dev)
        dist.all_reduce(ms, op=dist.ReduceOp.MAX)
        dist.barrier()
        nt, nx = E.pde_streams(pd)
        K = 1 + nt + nx
        tf = 3 * K * prog.flops_per_point() * N / (float(ms) * 1e-3) / 1e12
        out[tag] = {"workload": name, "global_points": int(N), "points_per_gpu": int(hi - lo), "n_gpus": world, "streams": K,
                    "ms_per_step": float(ms), "points_per_s": N / float(ms) * 1e3, "tflops_aggregate": tf,
                    "frac_of_n_gpu_peak": tf / (PEAK_F32_MFMA_TFLOPS * world),
                    "collective": f"1 all-reduce/step of the flat gradient ({flat.numel()} floats)",
                    "baseline_config": "configs[3]: 4xMI355X data-parallel" if tag == "C4" else "configs[4]: sharded 8xMI355X, loss all-reduce"}
        del net, eq, xs, ts_, flat, prog
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=50000,
                    help="requested collocation points: per GPU (weak) or in total (strong); uniform -> floor(sqrt)^2")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--spinup", type=int, default=0, help="extra untimed launches before the warm-up steps (experiments; "
                    "the sustained-clock figure is reported separately as `sustained`)")
    ap.add_argument("--full", action="store_true", help="also measure everything beside the headline figure (sustained "
                    "clock, CPU baseline, parity, training schedule, secondary / sharded configurations, strong scaling)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline, parity and training legs")
    ap.add_argument("--no-train", action="store_true", help="--full: skip the final-residual-L2 schedule")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the C1/C3/C4/C5 figures")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # PINN_BENCH_REHEARSAL=1: rehearse the N > 1 code path on a ONE-GPU box (all ranks on cuda:0, gloo instead of
    # RCCL, which refuses two ranks on one device).  Not a measurement mode.
    rehearsal = os.environ.get("PINN_BENCH_REHEARSAL") == "1"
    dev = torch.device("cuda:0" if rehearsal else f"cuda:{local}")
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from __graft_entry__ import _burgers
    from pinnrl_amd import _lib
    from pinnrl_amd import distributed as D
    from pinnrl_amd import engine as E

    cfg, model, pde = _burgers(dev, hidden=128, layers=4, mapping=32, scale=10.0, seed=0)  # identical theta_0 on every rank
    strong = args.scaling == "strong"
    # synthetic points from the PRODUCT sampler on the device (pde_base.py:806-860 restated there): a rank-specific
    # seed under weak scaling, one shared seed (identical global batch, then contiguous shards) under strong scaling
    torch.manual_seed(1 if strong else 1 + rank)
    xg, tg = pde.generate_collocation_points(args.points, strategy="uniform")
    n_global = xg.shape[0] if strong else xg.shape[0] * world
    if strong:
        lo, hi = D.shard_bounds(xg.shape[0], rank, world)
        x, t = xg[lo:hi].contiguous(), tg[lo:hi].contiguous()
    else:
        x, t = xg, tg
    N = x.shape[0]
    prog = model.program()
    pd = pde._pde_desc()
    _, n_grad = prog.grad_layout()
    buf = torch.zeros(n_grad + 4, dtype=torch.float32, device=dev)  # [flat gradient || loss sum || pad]
    flat, loss_sum = buf[:n_grad], buf[n_grad : n_grad + 1]

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]

    def step(i=None):
        buf.zero_()
        if i is not None:
            ev[i][0].record()
        E.residual_loss_grad(prog, pd, x, t, 1.0 / n_global, flat, loss_sum=loss_sum)
        if i is not None:
            ev[i][1].record()
        if world > 1:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM)

    # (--spinup N: extra untimed launches, off by default — the driver's --warmup means what it says.  The first few
    # dozen launches after an idle period run below the sustained clock; that figure is measured AFTER the timed region
    # and reported separately as `sustained`.)
    for _ in range(args.spinup):
        step()
    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax)
    kern_ms = sum(a.elapsed_time(b) for a, b in ev) / args.steps
    if args.dump_outputs and rank == 0:  # before any later launch reuses buf
        import numpy as np

        os.makedirs(args.dump_outputs, exist_ok=True)
        grad = torch.cat([g.flatten() for g in E.split_flat_grad(prog, flat) if g is not None])  # trainable, unpadded
        np.save(os.path.join(args.dump_outputs, "grad.npy"), grad.cpu().numpy().astype(np.float32))
        np.save(os.path.join(args.dump_outputs, "loss_sum.npy"), loss_sum.cpu().numpy().astype(np.float32))
    # sustained-clock figure, outside the timed region: 100 more launches, then 50 timed ones
    sustained = None
    if world == 1 and args.full:
        for _ in range(100):
            step()
        torch.cuda.synchronize()
        ts = time.perf_counter()
        for _ in range(50):
            step()
        torch.cuda.synchronize()
        sus_ms = 1e3 * (time.perf_counter() - ts) / 50
        sustained = {"after_untimed_launches": args.spinup + args.warmup + args.steps + 100, "steps": 50, "ms_per_step": sus_ms,
                     "value": n_global / sus_ms * 1e3}

    # north_star's ">= 6x strong scaling at 8 GPUs": beside the weak-scaling `value`, every N > 1 run also times ONE global
    # 10^6-point batch split over the ranks by shard_bounds (+ the all-reduce) against the same batch on rank 0 alone
    strong_fig = None
    if world > 1 and args.full:
        torch.manual_seed(7)  # identical on every rank
        xs, ts_ = pde.generate_collocation_points(1000000, strategy="uniform")
        ns = xs.shape[0]
        lo, hi = D.shard_bounds(ns, rank, world)

        def timed(xa, ta, reduce, reps=10):
            for _ in range(3):
                buf.zero_()
                E.residual_loss_grad(prog, pd, xa, ta, 1.0 / ns, flat, loss_sum=loss_sum)
                if reduce:
                    dist.all_reduce(buf, op=dist.ReduceOp.SUM)
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            for _ in range(reps):
                buf.zero_()
                E.residual_loss_grad(prog, pd, xa, ta, 1.0 / ns, flat, loss_sum=loss_sum)
                if reduce:
                    dist.all_reduce(buf, op=dist.ReduceOp.SUM)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t_0) / reps

        dist.barrier()
        ms_n = torch.tensor([timed(xs[lo:hi].contiguous(), ts_[lo:hi].contiguous(), True)], dtype=torch.float64, device=dev)
        dist.all_reduce(ms_n, op=dist.ReduceOp.MAX)
        dist.barrier()
        ms_1 = timed(xs, ts_, False) if rank == 0 else 0.0  # the other ranks idle meanwhile
        dist.barrier()
        strong_fig = {"points": int(ns), "ms_1": ms_1, "ms_N": float(ms_n), "speedup": (ms_1 / float(ms_n)) if rank == 0 else None,
                      "n_gpus": world, "note": "one global batch split by shard_bounds + 1 all-reduce of [grad || loss] per step, "
                                               "max over ranks, vs the same batch on rank 0 alone"}
        del xs, ts_

    sharded = None
    if world > 1 and args.full and not args.no_secondary:
        sharded = sharded_configs(E, D, dist, dev, rank, world)

    if rank == 0:
        K = 4
        flops_pt = 3 * K * prog.flops_per_point()  # forward jets + delta-propagation + weight-gradient GEMMs
        achieved = flops_pt * N / (kern_ms * 1e-3) / 1e12
        traffic, traffic_src = pmc_traffic()
        out = {
            "metric": "collocation-points/sec (residual+grad) + final residual L2, Burgers 1D",
            "value": n_global * args.steps / elapsed,
            "unit": "points/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": "BASELINE configs[1]: Burgers 1D nu=0.01/pi, fourier 4x128 tanh (41 473 params), "
                            + (f"ONE global batch of {n_global} collocation points split over {world} GPU(s)" if strong else
                               f"{N} collocation points per GPU ({args.points} requested, uniform -> floor(sqrt)^2)")
                            + ", residual + mean(r^2) + d/dtheta in one fused launch",
                "points_per_gpu": N, "global_points": n_global, "streams": K,
                "collective": "none" if world == 1 else f"1 all-reduce/step of [grad || loss] ({n_grad + 4} floats)",
                "sampler": "pde.generate_collocation_points(strategy='uniform') on the device",
                "untimed_launches": args.spinup + args.warmup,
            },
            "roofline": {
                "bound": "mfma", "achieved": achieved, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": achieved / PEAK_F32_MFMA_TFLOPS, "traffic": traffic,
                "traffic_source": (traffic_src + ": rocprofv3 FETCH_SIZE (x2) + WRITE_SIZE passes of this command, committed; not "
                                   "measured inside this run") if traffic_src else None,
                "kernel": "pinn::jet_kernel_wide<tanh, NT=1, NX=2, reverse>", "kernel_ms": kern_ms,
                "kernel_ms_covers": "the call's launches between events on the launch stream: the fused kernel (every workgroup "
                                    "stores its gradient row) and the fixed-order row sum (wide_rows_reduce)",
                "flops_per_point": flops_pt,
            },
            "sustained": sustained,
            "strong": strong_fig,
            "sharded": sharded,
            "residual_l2_theta0": math.sqrt(float(loss_sum) / n_global),
            "build_info": _lib.build_info() or "all kernel units in their preferred form",
        }
        if rehearsal:
            out["config"]["rehearsal"] = "all ranks on cuda:0 over gloo - code-path check, not a measurement"
        if world == 1 and args.full and not args.no_cpu:
            import oracle as O  # checker and CPU baseline only; never inside the timed region

            pspec = O.PdeSpec(name="burgers", parameters={"nu": 0.01 / math.pi})
            aspec = O.ArchSpec("fourier", hidden_dim=128, num_layers=4)
            sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
            x_cpu, t_cpu = x.cpu(), t.cpu()
            nthr = host_threads()
            v_all, n_all, L_cpu, g = cpu_eval(O, pspec, aspec, sd, x_cpu, t_cpu, args.cpu_seconds, nthr)
            v_one, n_one, _, _ = cpu_eval(O, pspec, aspec, sd, x_cpu, t_cpu, min(args.cpu_seconds, 6.0), 1)
            torch.set_num_threads(nthr)
            out["cpu_baseline"] = {
                "value": v_all, "unit": "points/s", "cores": nthr, "kind": "port", "cpu_model": cpu_model(),
                "value_1thread": v_one,
                "sample": f"best of {n_all} evaluations of the same {N}-point batch (~{args.cpu_seconds:.0f} s), fp32, torch "
                          f"{torch.__version__} CPU; 1-thread figure: best of {n_one}",
            }
            g_cpu = torch.cat([g[k].flatten() for k, _ in model.named_parameters()])
            g_gpu = torch.cat([gg.flatten().cpu() for gg, tr in zip(E.split_flat_grad(prog, flat), prog.trainable) if tr])
            out["parity"] = {
                "loss_rel_err": abs(float(loss_sum) / N - L_cpu) / abs(L_cpu),
                "grad_rel_l2": float((g_gpu - g_cpu).norm() / g_cpu.norm()),
                "residual_l2_cpu": math.sqrt(L_cpu),
            }
            out["speedup_vs_cpu"] = out["value"] / v_all
            # north_star's ">= 10x at 5k points": the reference's own CPU-runnable size (uniform: 5 000 -> 4 900)
            torch.manual_seed(4)
            x5, t5 = pde.generate_collocation_points(5000, strategy="uniform")
            v5_gpu = gpu_points_per_s(E, prog, pd, x5, t5, buf, n_grad)
            v5_cpu, _, _, _ = cpu_eval(O, pspec, aspec, sd, x5.cpu(), t5.cpu(), 3.0, nthr)
            out["points_5k"] = {"points": int(x5.shape[0]), "value": v5_gpu, "cpu_value": v5_cpu, "speedup_vs_cpu": v5_gpu / v5_cpu,
                                "note": "154 tiles on 256 CUs: launch- and occupancy-bound, see DESIGN.md"}
            if not args.no_train:
                out["training"] = training_parity(dev, O, pspec, aspec)
        if world == 1 and args.full and not args.no_secondary:
            out["secondary"] = secondary_configs(E)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
