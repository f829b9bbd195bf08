"""GPU parity beyond the committed fixtures: width 256 / 512, non-uniform widths, and the BASELINE networks at FULL
depth and width (fourier 4x128, resnet 6x256, siren 8x256, attention 4x128).

The golden fixtures stop at width 128, so these cases are pinned against the oracle evaluated on the fly in fp64 (the
oracle itself is pinned bit-for-bit to the reference by oracle/make_golden.py; networks with a LayerNorm are held to
its composite-LayerNorm path, the exact derivative — see tests/test_oracle_golden.py)."""

import math

import pytest
import torch

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(arch, pde_name, dim=1, **kw):
    import oracle as O

    spec = O.ArchSpec(architecture=arch, input_dim=dim + 1, hidden_dim=256, **kw)
    params = {"burgers": {"nu": 0.01 / math.pi}, "kdv": {}, "heat": {"alpha": 0.05}, "allen_cahn": {"epsilon": 0.05},
              "cahn_hilliard": {"epsilon": 0.05}}[pde_name]
    domain = {"kdv": ((-3.0, 3.0),)}.get(pde_name, ((-1.0, 1.0),) * dim)
    pde = O.PdeSpec(name=pde_name, dimension=dim, domain=domain, time_domain=(0.0, 1.0), parameters=params)
    sd = O.init_state_dict(spec, seed=11)
    torch.manual_seed(12)
    x, t = O.sample_uniform(pde, 230 if dim == 1 else 220)
    return spec, pde, sd, x[:201], t[:201]  # 7 tiles, the last one ragged


def _gpu(spec, pde, sd, x, t, dev):
    from hip_helpers import pde_desc_from_spec, program_from_spec
    from pinnrl_amd import engine as E

    prog, names = program_from_spec(spec, sd, dev)
    pd = pde_desc_from_spec(pde)
    flat = E.new_flat_grad(prog, dev)
    r, s = E.residual_loss_grad(prog, pd, x.to(dev), t.to(dev), 1.0 / x.shape[0], flat, want_residual=True)
    r_f, s_f = E.residual_forward(prog, pd, x.to(dev), t.to(dev))
    assert torch.equal(r_f, r), "forward-only and fused launches must agree bit for bit"
    grads = {n: g for n, g in zip(names, E.split_flat_grad(prog, flat)) if g is not None}
    return r.cpu(), float(s) / x.shape[0], grads


def _oracle64(spec, pde, sd, x, t, layer_norm="composite"):
    import oracle as O

    sd64 = {k: v.double() for k, v in sd.items()}
    return O.residual_loss_and_grad(pde, spec, sd64, x.double(), t.double(), layer_norm=layer_norm)


def _per_tensor(g, g_o, what, spec, pde, sd, x, t):
    """Tensor by tensor at hip_helpers.TENSOR_TOL (the concatenated comparison lets a bias or a LayerNorm parameter hide
    behind the weight matrices); the fp32 floor of a tensor above it is the same oracle in fp32."""
    import oracle as O
    from hip_helpers import check_tensors

    def floor():
        return O.residual_loss_and_grad(pde, spec, {k: v.float() for k, v in sd.items()}, x.float(), t.float(), layer_norm="composite")[2]

    check_tensors(g, {k: v for k, v in g_o.items() if k in g}, what, floor)


@pytest.mark.parametrize("arch,pde_name,kw", [
    ("fourier", "burgers", dict(num_layers=3, mapping_size=32, scale=3.0)),             # K = 4, Fourier encoding
    ("siren", "kdv", dict(num_layers=3, omega_0=6.0)),                                    # K = 5, first Linear + sin
    ("feedforward", "heat", dict(num_layers=3, activation="gelu")),                       # K = 3, first Linear + gelu
])
def test_stream_serial_two_tile_kernel(arch, pde_name, kw, dev):
    spec, pde, sd, x, t = _case(arch, pde_name, **kw)
    r, L, g = _gpu(spec, pde, sd, x, t, dev)
    r_o, L_o, g_o = _oracle64(spec, pde, sd, x, t)
    assert rel_l2(r, r_o) <= TOL
    assert abs(L - float(L_o)) <= TOL * abs(float(L_o))
    keys = [k for k in g_o if k in g]
    got = torch.cat([g[k].flatten().cpu() for k in keys])
    want = torch.cat([g_o[k].flatten() for k in keys])
    e_g = rel_l2(got, want, label="gradient", tol=TOL)
    assert e_g <= TOL, f"{e_g:.3e}"
    _per_tensor(g, g_o, f"{arch} 3x256 {pde_name}", spec, pde, sd, x, t)


def test_resnet_width_256(dev):
    """ResNet at width 256: residual and gradient vs the oracle's composite-LayerNorm path (the exact derivative); the
    reference's fused-layer_norm gradient is off by torch's third-derivative error and only bounded."""
    spec, pde, sd, x, t = _case("resnet", "allen_cahn", num_layers=2, num_blocks=2, activation="tanh")
    r, L, g = _gpu(spec, pde, sd, x, t, dev)
    r_o, L_o, g_o = _oracle64(spec, pde, sd, x, t)
    assert rel_l2(r, r_o) <= TOL
    keys = [k for k in g_o if k in g]
    got = torch.cat([g[k].flatten().cpu() for k in keys])
    exact = torch.cat([g_o[k].flatten() for k in keys])
    assert rel_l2(got, exact) <= TOL, f"{rel_l2(got, exact):.3e}"
    _, _, g_f = _oracle64(spec, pde, sd, x, t, layer_norm="fused")
    assert rel_l2(got, torch.cat([g_f[k].flatten() for k in keys])) <= 5e-4  # witness of the library error
    _per_tensor(g, g_o, "resnet 2x256 allen_cahn", spec, pde, sd, x, t)


def test_attention_width_256(dev):
    spec, pde, sd, x, t = _case("attention", "cahn_hilliard", dim=2, num_layers=2, activation="gelu", num_heads=4)
    r, L, g = _gpu(spec, pde, sd, x, t, dev)
    r_o, L_o, g_o = _oracle64(spec, pde, sd, x, t)
    assert rel_l2(r, r_o) <= TOL
    keys = [k for k in g_o if k in g]
    got = torch.cat([g[k].flatten().cpu() for k in keys])
    want = torch.cat([g_o[k].flatten() for k in keys])
    assert rel_l2(got, want) <= TOL, f"{rel_l2(got, want):.3e}"
    _per_tensor(g, g_o, "attention 2x256 cahn_hilliard 2-D", spec, pde, sd, x, t)


@pytest.mark.parametrize("arch,kw", [
    ("fourier", dict(num_layers=3, mapping_size=32, scale=3.0)),
    ("siren", dict(num_layers=3, omega_0=6.0)),
    ("resnet", dict(num_layers=2, num_blocks=2, activation="tanh")),
])
def test_value_stream_backward_at_width_256(arch, kw, dev):
    """The K = 1 launches behind `model(inp)` and its backward (boundary / initial terms of compute_loss): u and
    d<c, u>/d(theta) for an arbitrary cotangent c, against torch autograd through the oracle's forward in fp64."""
    import oracle as O
    from hip_helpers import program_from_spec
    from pinnrl_amd import engine as E

    spec, pde, sd, x, t = _case(arch, "burgers", **kw)
    prog, names = program_from_spec(spec, sd, dev)
    torch.manual_seed(40)
    cot = torch.randn(1, x.shape[0])
    u = E.jets_forward(prog, x.to(dev), t.to(dev), 0, 0)
    flat = E.new_flat_grad(prog, dev)
    E.jets_backward(prog, x.to(dev), t.to(dev), 0, 0, cot.to(dev), flat)
    params = {k: v.double().requires_grad_(k != "model.fourier.B") for k, v in sd.items()}
    u_o = O.network_forward(spec, params, torch.cat([x, t], 1).double())
    assert rel_l2(u[0].cpu(), u_o.detach().squeeze(1)) <= TOL
    keys = [k for k in params if params[k].requires_grad]
    g_o = torch.autograd.grad((u_o.squeeze(1) * cot[0].double()).sum(), [params[k] for k in keys])
    got = {n: g for n, g in zip(names, E.split_flat_grad(prog, flat)) if g is not None}
    a = torch.cat([got[k].flatten().cpu() for k in keys])
    b = torch.cat([g.flatten() for g in g_o])
    assert rel_l2(a, b) <= TOL, f"{rel_l2(a, b):.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE networks at full depth and width: d(mean r^2)/d(theta) against the fp64 oracle on 256 points
# ---------------------------------------------------------------------------------------------------------------------
def _full(arch, pde_name, dim=1, n=256, **kw):
    import oracle as O

    spec = O.ArchSpec(architecture=arch, input_dim=dim + 1, **kw)
    params = {"burgers": {"nu": 0.01 / math.pi}, "kdv": {}, "heat": {"alpha": 0.01}, "allen_cahn": {"epsilon": 0.01},
              "cahn_hilliard": {"epsilon": 0.01}}[pde_name]
    domain = {"kdv": ((-15.0, 15.0),), "heat": ((0.0, 1.0),), "cahn_hilliard": ((0.0, 1.0),) * dim}.get(pde_name, ((-1.0, 1.0),) * dim)
    tdom = (0.0, 5.0) if pde_name == "kdv" else (0.0, 1.0)
    pde = O.PdeSpec(name=pde_name, dimension=dim, domain=domain, time_domain=tdom, parameters=params)
    sd = O.init_state_dict(spec, seed=0)
    torch.manual_seed(1)
    x, t = O.sample_uniform(pde, 289 if dim == 1 else 300)
    return spec, pde, sd, x[:n].contiguous(), t[:n].contiguous()


@pytest.mark.parametrize("name,arch,pde_name,dim,kw", [
    ("C1 heat / fourier 4x128", "fourier", "heat", 1, dict(hidden_dim=128, num_layers=4)),
    ("C2 burgers / fourier 4x128", "fourier", "burgers", 1, dict(hidden_dim=128, num_layers=4)),
    ("C3 allen-cahn / resnet 6x256", "resnet", "allen_cahn", 1, dict(hidden_dim=256, num_layers=6, num_blocks=6)),
    ("C4 kdv / siren 8x256", "siren", "kdv", 1, dict(hidden_dim=256, num_layers=8, omega_0=30.0)),
    ("C5 cahn-hilliard 2-D / attention 4x128", "attention", "cahn_hilliard", 2,
     dict(hidden_dim=128, num_layers=4, activation="gelu", num_heads=4)),
    # first Linear behind three / two input columns at width 256 (its adjoint: lm_ew_bwd's per-feature sums)
    ("2-D input / feedforward 3x256", "feedforward", "cahn_hilliard", 2, dict(hidden_dim=256, num_layers=3, activation="tanh")),
    ("1-D input / feedforward gelu 3x256", "feedforward", "burgers", 1, dict(hidden_dim=256, num_layers=3, activation="gelu")),
])
def test_baseline_networks_full_depth_gradient(name, arch, pde_name, dim, kw, dev):
    """the weight gradient of the five BASELINE networks at their full depth and width, through the
    C ABI, against the fp64 oracle (not a self-comparison).  All five at the north-star tolerance: the 8-layer SIREN
    (third derivatives, omega_0 = 30) measures 3.4e-6 / 4.7e-6 on residual / gradient through the fused kernels and
    4.4e-6 / 5.9e-6 unfused (profiles/parity_r03.md; round 2 held it to 2e-5 without recording the margin)."""
    spec, pde, sd, x, t = _full(arch, pde_name, dim, **kw)
    r, L, g = _gpu(spec, pde, sd, x, t, dev)
    r_o, L_o, g_o = _oracle64(spec, pde, sd, x, t)
    tol = TOL
    e_r = rel_l2(r, r_o, label="residual", tol=tol)
    assert e_r <= tol, f"{name}: residual {e_r:.3e}"
    assert rel_err(L, float(L_o), label="loss", tol=tol) <= tol
    keys = [k for k in g_o if k in g]
    assert len(keys) == len(g_o)
    got = torch.cat([g[k].flatten().cpu() for k in keys])
    want = torch.cat([g_o[k].flatten() for k in keys])
    e_g = rel_l2(got, want, label="gradient", tol=tol)
    assert e_g <= tol, f"{name}: gradient {e_g:.3e}"
    for k in keys:  # and tensor by tensor, so that one small tensor cannot hide behind a large one
        if float(g_o[k].norm()) > 1e-12:
            assert rel_l2(g[k].cpu(), g_o[k]) <= 10 * tol, f"{name}: {k} {rel_l2(g[k].cpu(), g_o[k]):.3e}"
    _per_tensor(g, g_o, name, spec, pde, sd, x, t)


@pytest.mark.parametrize("arch,pde_name,kw", [
    ("feedforward", "burgers", dict(hidden_dims=[64, 128, 32], activation="tanh")),      # non-uniform widths
    ("feedforward", "burgers", dict(hidden_dims=[128, 64, 96], activation="tanh")),
    ("feedforward", "burgers", dict(hidden_dims=[50, 70, 33], activation="gelu")),       # nothing a multiple of 32
    ("feedforward", "burgers", dict(hidden_dim=512, num_layers=2, activation="tanh")),   # config.yaml:16,27
    ("resnet", "allen_cahn", dict(hidden_dim=512, num_layers=1, num_blocks=1, activation="tanh")),
    ("feedforward", "burgers", dict(hidden_dim=384, num_layers=2, activation="tanh")),   # depth 384: lm_gemm_wres16<12>
    # 13 Linears of 512 x 512 = 52 blocks of 256 x 256: more than one batched weight-gradient launch holds (48 jobs)
    ("feedforward", "burgers", dict(hidden_dim=512, num_layers=14, activation="tanh")),
    ("feedforward", "kdv", dict(hidden_dim=124, num_layers=3, activation="tanh", layer_norm=True)),  # YAML default shape
    ("siren", "kdv", dict(hidden_dims=[124, 124], omega_0=6.0)),
    # LayerNorm widths between the tested 128 and 256: 6 / 10 / 13 waves per workgroup in the element-wise kernels and
    # in the LDS-DMA prefetch of the LayerNorm adjoint (pieces = K * Hp / 16 per record)
    ("resnet", "allen_cahn", dict(hidden_dim=96, num_layers=2, num_blocks=2, activation="tanh")),
    ("resnet", "burgers", dict(hidden_dim=160, num_layers=2, num_blocks=2, activation="gelu")),
    ("attention", "burgers", dict(hidden_dim=200, num_layers=2, num_heads=4, activation="gelu")),
])
@pytest.mark.parametrize("engine", ["default", "lm"])
def test_arbitrary_widths(arch, pde_name, kw, engine, dev):
    """Hidden widths that are not multiples of 32, differ per layer, or exceed 256 (reference defaults: 124 and 512,
    pinnrl/config/config.yaml:16,22,27,35) — packed and zero-padded by the layer-major engine."""
    import oracle as O
    from hip_helpers import pde_desc_from_spec, program_from_spec
    from pinnrl_amd import engine as E

    kw = dict(kw)
    if "hidden_dims" in kw:
        kw.setdefault("hidden_dim", kw["hidden_dims"][0])
        kw.setdefault("num_layers", len(kw["hidden_dims"]))
    spec = O.ArchSpec(architecture=arch, **kw)
    params = {"burgers": {"nu": 0.02}, "kdv": {}, "allen_cahn": {"epsilon": 0.05}}[pde_name]
    domain = ((-3.0, 3.0),) if pde_name == "kdv" else ((-1.0, 1.0),)
    pde = O.PdeSpec(name=pde_name, domain=domain, parameters=params)
    sd = O.init_state_dict(spec, seed=61)
    torch.manual_seed(62)
    x, t = O.sample_uniform(pde, 150)
    x, t = x[:131].contiguous(), t[:131].contiguous()
    r_o, L_o, g_o = _oracle64(spec, pde, sd, x, t)
    prog, names = program_from_spec(spec, sd, dev)
    prog.set_layer_major(engine == "lm")
    pd = pde_desc_from_spec(pde)
    flat = E.new_flat_grad(prog, dev)
    r, s = E.residual_loss_grad(prog, pd, x.to(dev), t.to(dev), 1.0 / x.shape[0], flat, want_residual=True)
    e_r = rel_l2(r.cpu(), r_o, label="residual", tol=TOL)
    assert e_r <= TOL, f"{e_r:.3e}"
    by_name = {n: g for n, g in zip(names, E.split_flat_grad(prog, flat)) if g is not None}
    keys = [k for k in g_o if k in by_name]
    got = torch.cat([by_name[k].flatten().cpu() for k in keys])
    want = torch.cat([g_o[k].flatten() for k in keys])
    assert rel_l2(got, want) <= TOL, f"{rel_l2(got, want):.3e}"


def test_deterministic_mode_at_width_256(dev):
    """PINN_FLAG_DETERMINISTIC through the 256 x 256 weight-gradient kernel (LDS-DMA staging, per-split partial blocks)
    and the LayerNorm element-wise kernels: two launches bit-identical, equal to the default path to rounding, on a
    batch large enough for several column blocks per workgroup."""
    from hip_helpers import pde_desc_from_spec, program_from_spec
    from pinnrl_amd import engine as E
    import oracle as O

    spec = O.ArchSpec(architecture="resnet", input_dim=2, hidden_dim=256, num_layers=2, num_blocks=2)
    pde = O.PdeSpec(name="allen_cahn", parameters={"epsilon": 0.05})
    sd = O.init_state_dict(spec, seed=21)
    torch.manual_seed(22)
    x, t = O.sample_uniform(pde, 40000)
    x, t = x.to(dev), t.to(dev)
    prog, names = program_from_spec(spec, sd, dev)
    pd = pde_desc_from_spec(pde)
    N = x.shape[0]
    ref = E.new_flat_grad(prog, dev)
    _, s_ref = E.residual_loss_grad(prog, pd, x, t, 1.0 / N, ref)
    prog.set_deterministic(True)
    runs = []
    for _ in range(2):
        flat = E.new_flat_grad(prog, dev)
        _, s_ = E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat)
        runs.append((flat.clone(), s_.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert rel_l2(runs[0][0].cpu(), ref.cpu()) <= TOL
    assert abs(float(runs[0][1]) - float(s_ref)) <= TOL * abs(float(s_ref))


@pytest.mark.parametrize("arch,pde_name,kw", [
    ("attention", "burgers", dict(hidden_dim=128, num_layers=1, num_heads=4, activation="gelu")),   # depth-512 GEMMs, 128-wide dW blocks
    ("attention", "allen_cahn", dict(hidden_dim=96, num_layers=1, num_heads=4, activation="gelu")), # depth 384
    ("siren", "kdv", dict(hidden_dim=512, num_layers=2, omega_0=6.0)),                              # depth 512 x 512 rows
    ("resnet", "allen_cahn", dict(hidden_dim=256, num_layers=1, num_blocks=1, activation="tanh")),  # 256 x 256 dW blocks, batched
], ids=["attention128", "attention96", "siren512", "resnet256"])
def test_steady_state_of_the_persistent_gemm_loops(arch, pde_name, kw, dev):
    """The persistent GEMM kernels (lm_gemm_wres16 / lm_gemm_wres, lm_fused, the batched dW launches) double-buffer their
    staged blocks and hand finished tiles over to the next loop iteration; at the fixture sizes every workgroup gets ONE
    block, so that hand-over never runs.  Here one launch over 40 000 points (up to 20 blocks per workgroup) must equal
    the sum of 20 launches over 2 000-point slices (at most one block per workgroup): per-point residuals bit for bit
    — they do not depend on which workgroup or loop iteration computes them —, loss and gradient to rounding; and the
    residuals of a sample of points must match the fp64 oracle."""
    import oracle as O
    from hip_helpers import pde_desc_from_spec, program_from_spec
    from pinnrl_amd import engine as E

    spec = O.ArchSpec(architecture=arch, **kw)
    params = {"burgers": {"nu": 0.02}, "kdv": {}, "allen_cahn": {"epsilon": 0.05}}[pde_name]
    domain = ((-3.0, 3.0),) if pde_name == "kdv" else ((-1.0, 1.0),)
    pde = O.PdeSpec(name=pde_name, domain=domain, parameters=params)
    sd = O.init_state_dict(spec, seed=81)
    torch.manual_seed(82)
    N, S = 40000, 2000
    x = ((torch.rand(N, 1) * 2 - 1) * domain[0][1]).to(dev)
    t = torch.rand(N, 1).to(dev)
    prog, names = program_from_spec(spec, sd, dev)
    prog.set_layer_major(True)
    pd = pde_desc_from_spec(pde)
    flat = E.new_flat_grad(prog, dev)
    r, s = E.residual_loss_grad(prog, pd, x, t, 1.0 / N, flat, want_residual=True)
    parts, fsum, ssum = [], E.new_flat_grad(prog, dev), 0.0
    for lo in range(0, N, S):
        rp, sp = E.residual_loss_grad(prog, pd, x[lo:lo + S].contiguous(), t[lo:lo + S].contiguous(), 1.0 / N, fsum, want_residual=True)
        parts.append(rp)
        ssum += float(sp)
    assert torch.equal(torch.cat(parts), r), "per-point residuals differ between one launch and per-slice launches"
    assert abs(float(s) - ssum) <= 2e-5 * abs(ssum)
    e_g = rel_l2(flat.cpu(), fsum.cpu(), label="gradient, one launch vs slices", tol=2e-5)
    assert e_g <= 2e-5, f"{e_g:.3e}"
    idx = torch.linspace(0, N - 1, 300).long()
    sd64 = {k: v.double() for k, v in sd.items()}
    r_o = O.compute_residual(pde, lambda inp: O.network_forward(spec, sd64, inp, "composite"), x[idx.to(dev)].cpu().double(),
                             t[idx.to(dev)].cpu().double()).detach()
    e_r = rel_l2(r[idx.to(dev)].cpu(), r_o, label="residual sample", tol=TOL)
    assert e_r <= TOL, f"{e_r:.3e}"


@pytest.mark.parametrize("arch,pde_name,kw,n,tol", [
    ("attention", "cahn_hilliard", dict(hidden_dim=32, num_layers=2, num_heads=4, activation="gelu"), 33, TOL),
    # one of these five points sits where a LayerNorm's variance is small: torch fp32 autograd on the CPU is 5e-4 from fp64
    # there (this path 2e-4); what the case checks is the 27 lanes beyond the batch
    ("attention", "kdv", dict(hidden_dim=64, num_layers=2, num_heads=2, activation="tanh"), 5, 1e-3),
    ("resnet", "cahn_hilliard", dict(hidden_dim=64, num_layers=2, num_blocks=2, activation="tanh"), 1, TOL),
], ids=["attention-ch4-2x32-N33", "attention-kdv-2x64-N5", "resnet-ch4-N1"])
def test_ragged_last_tile_under_layer_norm(arch, pde_name, kw, n, tol, dev):
    """Found by tools/fuzz_parity.py: the lanes of the last tile beyond the batch used to run on zero coordinates.  With the
    reference's zero-initialised first bias every feature of such a lane is equal, a LayerNorm there divides by sqrt(eps),
    its high-order jets overflow fp32 after a few layers, and 0 (their cotangent) x inf = NaN reached every weight
    gradient.  They now repeat the last point (lm_ew.h::load_coords)."""
    import oracle as O
    from hip_helpers import pde_desc_from_spec, program_from_spec
    from pinnrl_amd import engine as E

    spec = O.ArchSpec(architecture=arch, input_dim=2, **kw)
    dom = ((-3.0, 3.0),) if pde_name == "kdv" else ((-1.0, 1.0),)
    pde = O.PdeSpec(name=pde_name, dimension=1, domain=dom, time_domain=(0.0, 1.0),
                    parameters={"kdv": {}, "cahn_hilliard": {"epsilon": 0.05}}[pde_name])
    sd = O.init_state_dict(spec, seed=1)
    torch.manual_seed(1)
    x, t = O.sample_uniform(pde, max(n, 4) * 2)
    x, t = x[:n].contiguous(), t[:n].contiguous()
    r_o, L_o, g_o = _oracle64(spec, pde, sd, x, t)
    prog, names = program_from_spec(spec, sd, dev)
    pd = pde_desc_from_spec(pde)
    flat = E.new_flat_grad(prog, dev)
    r, s = E.residual_loss_grad(prog, pd, x.to(dev), t.to(dev), 1.0 / n, flat, want_residual=True)
    assert torch.isfinite(flat).all(), "non-finite weight gradient"
    assert rel_l2(r.cpu(), r_o, label="residual", tol=tol) <= tol
    by = {k: g for k, g in zip(names, E.split_flat_grad(prog, flat)) if g is not None}
    keys = [k for k in g_o if k in by]
    got = torch.cat([by[k].flatten().cpu() for k in keys])
    want = torch.cat([g_o[k].flatten() for k in keys])
    e_g = rel_l2(got, want, label="gradient", tol=tol)
    assert e_g <= tol, f"{e_g:.3e}"


def test_deterministic_mode_with_one_wide_layers(dev):
    """Found by tools/fuzz_parity.py: a 1 x H GEMM weight used to be packed as a vector, so the 32 x 32 block the
    weight-gradient kernels own behind dW ran over the following items of the packed gradient; with PINN_FLAG_DETERMINISTIC the
    reduction's plain `+= 0` on those addresses raced with the `+= db` of the bias stored there and lost it about every
    second call.  100 calls must be bit-identical and match the oracle."""
    import oracle as O
    from hip_helpers import pde_desc_from_spec, program_from_spec
    from pinnrl_amd import engine as E

    spec = O.ArchSpec(architecture="fourier", input_dim=2, hidden_dim=1, num_layers=4, mapping_size=8, scale=1.0, activation="tanh")
    pde = O.PdeSpec(name="kdv", dimension=1, domain=((-3.0, 3.0),), time_domain=(0.0, 1.0), parameters={})
    sd = O.init_state_dict(spec, seed=3)
    torch.manual_seed(3)
    x, t = O.sample_uniform(pde, 10)
    x, t = x[:5].contiguous(), t[:5].contiguous()
    r_o, L_o, g_o = _oracle64(spec, pde, sd, x, t)
    prog, names = program_from_spec(spec, sd, dev)
    prog.set_deterministic(True)
    pd = pde_desc_from_spec(pde)
    xd, td = x.to(dev), t.to(dev)
    first = None
    for _ in range(100):
        flat = E.new_flat_grad(prog, dev)
        E.residual_loss_grad(prog, pd, xd, td, 1.0 / 5, flat)
        if first is None:
            first = flat.clone()
        assert torch.equal(flat, first), "deterministic mode: two calls differ"
    by = {k: g for k, g in zip(names, E.split_flat_grad(prog, first)) if g is not None}
    for k in g_o:
        if k in by:
            assert rel_l2(by[k].cpu(), g_o[k]) <= TOL, k
