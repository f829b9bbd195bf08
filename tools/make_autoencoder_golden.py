"""Record the reference's AutoEncoder (pinnrl/neural_networks/autoencoder.py) on three small cases.

    python tools/make_autoencoder_golden.py /path/to/the/reference/checkout

Runs only where the reference package is present; no test imports this file.  Writes tests/golden/<tag>.npz per case
(tests/autoencoder_model.py::load_fixture reads them; they are deliberately NOT in tests/golden/manifest.json, whose keys
parametrise the oracle tests).  Each case is self-describing: `meta` is a JSON string in a 0-d unicode array, so
allow_pickle=False loads it.  Arrays:

    sd::<key>         fp32  theta_0 of the reference under meta["seed"], then every 1-D tensor perturbed
                            (autoencoder_model.perturb: biases and LayerNorm parameters, so that no term vanishes)
    x, t              fp32  (N, 1) points, uniform in the PDE's domain
    jets64            fp64  (K, N) [u, u_t, u_x, u_xx, ...] by autograd of autograd, LayerNorm written out
    residual64, loss64, grad64                 the reference's PDE class on the fp64 model, as the reference computes them
    residual64_exact, loss64_exact, grad64_exact   the same with torch.nn.functional.layer_norm replaced by
                            (x - mean) / sqrt(var + eps) * g + b while they run: torch's fused layer_norm differentiated three
                            times (the weight gradient of u_xx) is not exact; the GPU is held to these

Both gradients are kept for every case: `grad64_exact` is the parity target, `grad64` the witness that the distance between
the product and the reference is torch's fused-LayerNorm error and nothing else (tests/test_autoencoder_gpu.py asserts the
GPU's distance to it against the recorded one, tests/test_autoencoder_cpu.py the recorded distance itself).

A case larger than one committed file may be (1 MiB) is split over <tag>.npz, <tag>.1.npz, ... with long arrays cut into
name@@0, name@@1, ... pieces: at the shipped configuration's shape ONE fp64 gradient (142 293 parameters, 1.1 MB) is already
over the limit, so that case needs the pieces with or without `grad64`.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
import autoencoder_model as AM  # noqa: E402

FILE_BUDGET = 900 * 1024  # bytes of array data per file: under the 1 MiB limit with the zip directory on top

CASES = [
    dict(tag="autoencoder_burgers_tanh_ln_32_64_l16", seed=101, n_points=197,
         model=dict(input_dim=2, hidden_dims=[32, 64], latent_dim=16, activation="tanh", layer_norm=True, dropout=0.0, output_dim=1),
         pde=dict(name="burgers", domain=[[-1.0, 1.0]], time_domain=[0.0, 1.0], parameters={"nu": 0.05},
                  initial_condition={"type": "sine", "amplitude": -1.0, "frequency": 1.0})),
    dict(tag="autoencoder_kdv_gelu_33_l7", seed=102, n_points=203,
         model=dict(input_dim=2, hidden_dims=[33], latent_dim=7, activation="gelu", layer_norm=False, dropout=0.0, output_dim=1),
         pde=dict(name="kdv", domain=[[-3.0, 3.0]], time_domain=[0.0, 1.0], parameters={"speed": 1.0},
                  initial_condition={"type": "soliton", "speed": 1.0})),
    dict(tag="autoencoder_allen_cahn_relu_ln_default", seed=103, n_points=199,
         model=dict(input_dim=2, hidden_dims=[124, 248, 124], latent_dim=64, activation="relu", layer_norm=True, dropout=0.0, output_dim=1),
         pde=dict(name="allen_cahn", domain=[[-1.0, 1.0]], time_domain=[0.0, 1.0], parameters={"epsilon": 0.3},
                  initial_condition={"type": "tanh", "epsilon": 0.1})),
]
PERTURB = dict(seed_offset=7, scale=0.1)
STREAMS = {"burgers": (1, 2), "kdv": (1, 3), "allen_cahn": (1, 2)}


def composite_layer_norm(x, normalized_shape, weight=None, bias=None, eps=1e-5):
    dims = tuple(range(-len(normalized_shape), 0))
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps)
    if weight is not None:
        y = y * weight
    if bias is not None:
        y = y + bias
    return y


class composite_ln:
    def __enter__(self):
        self.saved = torch.nn.functional.layer_norm
        torch.nn.functional.layer_norm = composite_layer_norm

    def __exit__(self, *exc):
        torch.nn.functional.layer_norm = self.saved


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def jets_by_autograd(model, x, t, nt, nx):
    x = x.clone().requires_grad_(True)
    t = t.clone().requires_grad_(True)
    u = model(torch.cat([x, t], 1))
    out, d = [u], u
    for _ in range(nt):
        d = torch.autograd.grad(d.sum(), t, create_graph=True)[0]
        out.append(d)
    d = u
    for _ in range(nx):
        d = torch.autograd.grad(d.sum(), x, create_graph=True)[0]
        out.append(d)
    return torch.stack([o.detach()[:, 0] for o in out])


def write_split(tag, out_dir, arrays):
    """Greedy split over files of at most FILE_BUDGET bytes of data; arrays longer than that are cut along axis 0."""
    pieces = []
    for k, v in arrays.items():
        if v.nbytes <= FILE_BUDGET // 2:
            pieces.append((k, v))
            continue
        assert v.ndim == 1, k
        per = (FILE_BUDGET // 2) // v.itemsize
        for i, lo in enumerate(range(0, v.shape[0], per)):
            pieces.append((f"{k}@@{i}", v[lo:lo + per]))
    files, cur, size = [], {}, 0
    for k, v in pieces:
        if cur and size + v.nbytes > FILE_BUDGET:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    files.append(cur)
    paths = []
    for i, content in enumerate(files):
        path = os.path.join(out_dir, tag + (".npz" if i == 0 else f".{i}.npz"))
        np.savez_compressed(path, **content)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        paths.append(path)
    return paths


def run_case(case, AutoEncoder, PDEConfig, pde_cls, out_dir):
    tag, seed, m, p = case["tag"], case["seed"], case["model"], case["pde"]
    cpu = torch.device("cpu")
    torch.manual_seed(seed)
    net = AutoEncoder(dict(m, device=cpu))
    sd0 = {"model." + k: v.detach().clone() for k, v in net.state_dict().items()}
    sd = AM.perturb(sd0, seed + PERTURB["seed_offset"], PERTURB["scale"])
    net64 = AutoEncoder(dict(m, device=cpu)).double()
    net64.load_state_dict({k[len("model."):]: v.double() for k, v in sd.items()})

    gen = torch.Generator().manual_seed(seed + 1)
    N = case["n_points"]
    (xlo, xhi), (tlo, thi) = p["domain"][0], p["time_domain"]
    x = (xlo + (xhi - xlo) * torch.rand(N, 1, generator=gen)).float()
    t = (tlo + (thi - tlo) * torch.rand(N, 1, generator=gen)).float()
    x[0, 0], x[1, 0], t[0, 0], t[1, 0] = xlo, xhi, tlo, thi  # the domain's corners

    eq = pde_cls[p["name"]](config=PDEConfig(
        name=p["name"], domain=[tuple(d) for d in p["domain"]], time_domain=tuple(p["time_domain"]),
        parameters=dict(p["parameters"]), boundary_conditions={"dirichlet": {"type": "fixed", "value": 0.0}},
        initial_condition=dict(p["initial_condition"]), exact_solution={}, dimension=1, device=cpu))
    names = [k for k, _ in net64.named_parameters()]
    assert ["model." + k for k in names] == list(sd), "parameters are not the whole state_dict"

    def residual_loss_grad():
        net64.zero_grad()
        r = eq.compute_residual(net64, x.double(), t.double())
        L = eq._apply_loss_fn(r)
        L.backward()
        g = torch.cat([(q.grad if q.grad is not None else torch.zeros_like(q)).flatten() for _, q in net64.named_parameters()])
        return r.detach().numpy().copy(), np.float64(L.item()), g.numpy().copy()

    nt, nx = STREAMS[p["name"]]
    r64, L64, g64 = residual_loss_grad()
    with composite_ln():
        r64x, L64x, g64x = residual_loss_grad()
        jets = jets_by_autograd(net64, x.double(), t.double(), nt, nx).numpy()

    # the node-list restatement the engine implements, held to the exact arrays before anything is written
    meta = dict(tag=tag, seed=seed, perturb=dict(seed=seed + PERTURB["seed_offset"], scale=PERTURB["scale"]), model=m, pde=p,
                streams=[nt, nx], n_points=N, sd_keys=list(sd),
                grad64_vs_exact=dict(total=rel_l2(g64, g64x)), residual64_vs_exact=rel_l2(r64, r64x))
    off, worst = 0, ("", 0.0)
    for k, v in sd.items():
        n = v.numel()
        ge = g64x[off:off + n]
        e = rel_l2(g64[off:off + n], ge) if np.abs(ge).max() > 0 else float(np.abs(g64[off:off + n]).max())
        if e >= worst[1]:
            worst = (k, e)
        off += n
    meta["grad64_vs_exact"]["worst_tensor"], meta["grad64_vs_exact"]["worst"] = worst
    jn, rn, Ln, gn = AM.node_model_outputs(meta, sd, x, t)
    errs = dict(jets=max(rel_l2(jn[s], jets[s]) for s in range(1 + nt + nx)), residual=rel_l2(rn, r64x),
                loss=abs(Ln - L64x) / abs(L64x), grad=rel_l2(gn, g64x))
    assert max(errs.values()) <= 1e-12, (tag, errs)
    meta["node_model_vs_exact"] = errs

    arrays = {"meta": np.array(json.dumps(meta))}
    for k, v in sd.items():
        arrays["sd::" + k] = v.numpy()
    arrays.update(x=x.numpy(), t=t.numpy(), jets64=jets, residual64=r64, loss64=L64, residual64_exact=r64x, loss64_exact=L64x,
                  grad64_exact=g64x, grad64=g64)
    paths = write_split(tag, out_dir, arrays)
    print(f"{tag}: {sum(v.numel() for v in sd.values())} parameters, N = {N}; reference grad64 vs exact: total "
          f"{meta['grad64_vs_exact']['total']:.2e}, worst tensor {worst[0]} {worst[1]:.2e}; residual {meta['residual64_vs_exact']:.1e}; "
          f"node model vs exact: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items())
          + "; files " + ", ".join(f"{os.path.basename(q)} {os.path.getsize(q) // 1024} KB" for q in paths))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout that holds the pinnrl package")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(args.reference, "pinnrl")):
        sys.exit("the reference package is not there")
    sys.path.insert(0, args.reference)
    from pinnrl.neural_networks import AutoEncoder  # noqa: E402  (reference)
    from pinnrl.pdes.allen_cahn import AllenCahnEquation  # noqa: E402
    from pinnrl.pdes.burgers_equation import BurgersEquation  # noqa: E402
    from pinnrl.pdes.kdv_equation import KdVEquation  # noqa: E402
    from pinnrl.pdes.pde_base import PDEConfig  # noqa: E402

    for case in CASES:
        run_case(case, AutoEncoder, PDEConfig, {"burgers": BurgersEquation, "kdv": KdVEquation, "allen_cahn": AllenCahnEquation},
                 args.out)


if __name__ == "__main__":
    main()
