"""No GPU: the reference construction of tests/lm_chunk_cases.py.

That module compares an N-point launch, whose point i is distinct point i mod 203 and whose cotangents are random per index,
with fp64 autograd over the 203 distinct points alone — cotangents summed per distinct point, the loss weighted by the
counts.  Here fp64 autograd over all N points, with the same per-index cotangents, reproduces every quantity of that reference
to 1e-12 for one network; the direction case's jets are those of the sheared network of tests/direction_model.py; and the
declared cases are the matrix."""

import pytest
import torch

import direction_model as DM
import lm_chunk_cases as C

EXACT = 1e-12


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name,N", [("fourier_4x128_burgers", C.N_FULL), ("ff3_direction", C.N_ONE)])
def test_all_points_autograd_reproduces_the_distinct_point_reference(name, N):
    net = C.networks()[name]
    ref = C.reference(net, N)
    x, t = C.distinct_points(net)
    assert ref["idx"].tolist() == [i % C.P_DISTINCT for i in range(N)] and x.shape[0] == C.P_DISTINCT == 203
    # the cotangents are per index: two occurrences of the same distinct point carry different ones
    assert not torch.equal(ref["cot"][:, 0], ref["cot"][:, C.P_DISTINCT])
    assert torch.equal(ref["cot"], ref["cot"].float().double())
    idx = ref["idx"]
    full = C.reference(net, N, x=x[idx], t=t[idx], idx=torch.arange(N), like=ref)
    for s in range(ref["jets"].shape[0]):
        assert _rel(ref["jets"][s][idx], full["jets"][s]) <= EXACT, s
    assert _rel(ref["xg"], full["xg"]) <= EXACT and _rel(ref["tg"], full["tg"]) <= EXACT
    for k in ref["names"]:
        assert _rel(ref["adj"][k], full["adj"][k]) <= EXACT, k
    if net.pde is None:
        return
    assert _rel(ref["r"][idx], full["r"]) <= EXACT and _rel(ref["L"], full["L"]) <= EXACT
    assert torch.equal(ref["rbar"], ref["rbar"].float().double()) and ref["rbar"].shape == (N,)
    for k in ref["names"]:
        assert _rel(ref["gL"][k], full["gL"][k]) <= EXACT, k
        assert _rel(ref["gR"][k], full["gR"][k]) <= EXACT, k
    assert len(ref["dcoef"]) == len(C.COEFS[net.pde]) and _rel(ref["dcoef"], full["dcoef"]) <= EXACT


def test_direction_jets_are_those_of_the_sheared_network():
    """(sum_c d_c d/dx_c)^k u by autograd along the line equals the axis-0 derivative of the exactly sheared network
    (tests/direction_model.py) at the sheared coordinates."""
    import oracle as O

    net = C.networks()["ff3_direction"]
    x, t = C.distinct_points(net)
    params = {k: v.double() for k, v in C.state_dict(net).items()}
    jets = C.line_jets(net, params, x.double().requires_grad_(True), t.double().requires_grad_(True))
    sheared = DM.shear_state_dict(params, "model.layers.0.weight", net.direction)
    inp = DM.shear_inputs(torch.cat([x, t], 1).double(), net.direction)
    x0 = inp[:, :1].clone().requires_grad_(True)
    u = O.network_forward(net.spec, sheared, torch.cat([x0, inp[:, 1:]], 1), "composite")
    cur, want = u, [u[:, 0]]
    for _ in range(net.streams[1]):
        cur = torch.autograd.grad(cur, x0, torch.ones_like(cur), create_graph=True)[0]
        want.append(cur[:, 0])
    assert len(jets) == len(want) == 3
    for s in range(3):
        assert _rel(jets[s].detach(), want[s].detach()) <= EXACT, s


@pytest.mark.parametrize("name", C.NET_NAMES)
def test_no_output_is_a_one_point_comparison(name):
    """A relative L2 error over the indices of a launch says little when one distinct point carries the norm: every jet
    stream, the residual and both input cotangents spread over the points."""
    ref = C.reference(C.networks()[name], C.N_FULL)
    idx = ref["idx"]
    outputs = {f"jet stream {s}": j[idx] for s, j in enumerate(ref["jets"])}
    outputs.update(x_grad=ref["xg"].norm(dim=1), t_grad=ref["tg"][:, 0])
    if "r" in ref:
        outputs["residual"] = ref["r"][idx, 0]
    for what, v in outputs.items():
        per_point = torch.zeros(C.P_DISTINCT, dtype=torch.float64).index_add_(0, idx, v.double() ** 2)
        assert float(per_point.max() / per_point.sum()) <= C.MAX_SHARE, (what, float(per_point.max() / per_point.sum()))


def test_declared_cases():
    nets = C.networks()
    assert tuple(nets) == C.NET_NAMES and set(C.REDUCED) <= set(nets)
    full = [(n, N, d) for n, N, d in C.CASES if N == C.N_FULL]
    assert sorted(full) == sorted((n, C.N_FULL, d) for n in nets for d in (False, True))
    reduced = [(n, N, d) for n, N, d in C.CASES if N != C.N_FULL]
    assert sorted(reduced) == sorted((n, N, d) for n in C.REDUCED for N in (C.N_ONE, C.N_EXACT) for d in (False, True))
    assert C.N_CASES == len(C.CASES) + 1 == len(set(C.CASES)) + 1
    # three chunks with a ragged last tile of 7 points; a third chunk of one point; two exact chunks
    assert (C.N_FULL - 2 * C.CHUNK_POINTS) % 32 == 7 and C.N_ONE == 2 * C.CHUNK_POINTS + 1 and C.N_EXACT == 2 * C.CHUNK_POINTS
    assert C.P_DISTINCT % 2 == 1 and C.CHUNK_POINTS % C.P_DISTINCT == 18
    for net in nets.values():  # K round32(hmax) >= 128: the chunk is 64 tiles under a 1 MB record target
        K = 1 + sum(net.streams)
        widest = 160 if net.auto else max(max(net.spec.dims()), 4 * net.spec.hidden_dim if net.spec.architecture == "attention" else 0)
        assert K * ((widest + 31) // 32 * 32) >= 128, net.name
