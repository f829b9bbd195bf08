"""The layer-major variant matrix: the network list of tests/test_lm_variants_{cpu,gpu}.py, the variants a plan holds
(`pinn_lm_plan`), and the reachable matrix written out by enumeration.

A variant is one template instantiation of a layer-major kernel that a launch can select:

    ("lm_fused",      nt, nx, family, (nch, rt), ln, bwd, aux)      lm_fused_inst.hip
    ("lm_ew",         nt, nx, family, fpt,       ln, bwd, ew_kind)  lm_inst.hip: lm_ew_fwd (bwd 0), lm_ew_bwd (ew_kind 0),
                                                                    lm_ew_bwd_dma (ew_kind 1)
    ("lm_fourier_fwd", nt, nx, -1,    fpt,       0,  0,   2)
    ("lm_head",       nt, nx, -1,     fpt,       0,  bwd, -1)       bwd: lm_head seeds the cotangents in the same launch

family is the PinnAct id of the compiled family (0 tanh, 1 sin, 2 gelu, 3 sigmoid, 4 relu: leaky_relu, identity and
"no activation" run relu's).  The XG instantiations of lm_ew_bwd / lm_fourier_bwd (pinn_jet_backward_inputs) and the
space-only stream sets (0, 1) .. (0, 4) have their own tests (test_input_grad_gpu.py, test_axis_jets_gpu.py,
test_direction_jets_gpu.py) and are not part of this matrix.
"""

FUSED_SETS = [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]
SETS = FUSED_SETS + [(2, 0), (2, 2)]  # time order 2: element-wise units only, never fused (csrc/Makefile)
FAMILIES = ["tanh", "sin", "gelu", "sigmoid", "relu"]
FAM_ID = {"tanh": 0, "sin": 1, "gelu": 2, "sigmoid": 3, "relu": 4}
POLICIES = {"default": {}, "unfused": {"PINN_LM_FUSED": "0"}, "all_ln_fused": {"PINN_LM_FUSED_LN": "15"}}
N_PTS = 100  # three full 32-point tiles and a ragged one

A_DIMS = [128, 128, 128, 256, 256, 128]
F_MAPPING = {"tanh": 64, "gelu": 32, "sigmoid": 256, "relu": 512}  # 2 M Fourier features: 4, 1, 8 and 16 per thread
# C: the issue's 64, 512 and one layer wider than 512, in an order per family, so that the head (lm_head<FPT>) sees 1024,
# 64 and 512 features over the families of a stream set while every family keeps prologues of 1, 8 and 16 features per thread
C_DIMS = {"tanh": [64, 512, 1024], "sin": [1024, 512, 64], "gelu": [1024, 512, 64], "sigmoid": [64, 1024, 512], "relu": [64, 512, 1024]}


def networks(nt, nx, fam):
    """[(label, ArchSpec)] of one (stream set, family) case.

    A   feedforward (SIREN for sin) without LayerNorm, hidden_dims 128, 128, 128, 256, 256, 128: forward epilogues
        (4, 4), (4, 8), (8, 8) and reverse epilogues (4, 4), (8, 8), (4, 8) — the issue's 128, 128, 256, 256, 128 with one
        more 128 in front, because a reverse (4, 4) needs a 128 -> 128 node whose input is a record, not the coordinates.
    B   the same with LayerNorm (feedforward only: no reference architecture puts a LayerNorm before sin): LayerNorm
        epilogues forward and, at depth 128 (depth 256 under PINN_LM_FUSED_LN=15), in reverse; lm_ew_bwd_dma.
    C   widths 64, 512 and 1024 (C_DIMS) with and without LayerNorm: 1, 8 and 16 features per thread.
    F   Fourier features (the oracle's Fourier network has one hidden width: 128) of 128, 64, 512 and 1024 features by
        family, so that every stream set runs lm_fourier_fwd at 4, 1, 8 and 16 features per thread.
    R   ResNet (LayerNorm + skip record), two blocks, at widths 128 and 256 (the stream sets without fused units: 128
        only): the AUX records of the family.
    T   attention (add records, H -> 4 H gelu FFN, LayerNorm without activation), two layers, at widths 128 and 256.  Its
        fused nodes are the relu ("no activation") and gelu families' whatever the network's activation is, which only
        the first prologue sees: it runs once per fused stream set, in the gelu case.
    sin is SIREN's alone, so it has A and C (without LayerNorm) only."""
    import oracle as O

    if fam == "sin":
        return [("A", O.ArchSpec("siren", hidden_dims=A_DIMS, num_layers=len(A_DIMS), omega_0=3.0)),
                ("C", O.ArchSpec("siren", hidden_dims=C_DIMS[fam], num_layers=3, omega_0=3.0))]
    act = "leaky_relu" if (fam == "relu" and (nt, nx) == (1, 2)) else fam  # leaky_relu's slope on the relu units
    fused_set = (nt, nx) in FUSED_SETS
    nets = [("A", O.ArchSpec("feedforward", hidden_dims=A_DIMS, num_layers=len(A_DIMS), activation=act)),
            ("B", O.ArchSpec("feedforward", hidden_dims=A_DIMS, num_layers=len(A_DIMS), activation=act, layer_norm=True)),
            ("C", O.ArchSpec("feedforward", hidden_dims=C_DIMS[fam], num_layers=3, activation=act)),
            ("C_ln", O.ArchSpec("feedforward", hidden_dims=C_DIMS[fam], num_layers=3, activation=act, layer_norm=True)),
            ("F", O.ArchSpec("fourier", hidden_dim=128, num_layers=3, mapping_size=F_MAPPING[fam], scale=2.0, activation=act))]
    for h in (128, 256) if fused_set else (128,):
        nets.append((f"R{h}", O.ArchSpec("resnet", hidden_dim=h, num_layers=2, num_blocks=2, activation=act)))
        if fused_set and fam == "gelu":
            nets.append((f"T{h}", O.ArchSpec("attention", hidden_dim=h, num_layers=2, num_heads=4, activation=act)))
    return nets


def cases():
    """(nt, nx, family) of the matrix: every stream set of the element-wise units x every family."""
    return [(nt, nx, fam) for nt, nx in SETS for fam in FAMILIES]


def plan_variants(plan, nt, nx, backward):
    """The variants one plan (pinnrl_amd._lib.lm_plan) launches."""
    out = set()
    for rec in plan:
        fam, ln = rec["act_family"], rec["has_ln"]
        if rec["fwd_fused"]:
            out.add(("lm_fused", nt, nx, fam, (rec["fwd_nch"], rec["fwd_rt"]), ln, 0, rec["fwd_aux"]))
        elif rec["fwd_ew_kind"] == 2:
            out.add(("lm_fourier_fwd", nt, nx, -1, rec["fwd_fpt"], 0, 0, 2))
        elif rec["fwd_ew_kind"] == 0:
            out.add(("lm_ew", nt, nx, fam, rec["fwd_fpt"], ln, 0, 0))
        if rec["bwd_fused"]:
            out.add(("lm_fused", nt, nx, fam, (rec["bwd_nch"], rec["bwd_rt"]), ln, 1, rec["bwd_aux"]))
        elif rec["bwd_ew_kind"] in (0, 1):
            out.add(("lm_ew", nt, nx, fam, rec["bwd_fpt"], ln, 1, rec["bwd_ew_kind"]))
        if rec["head_fpt"] >= 0:
            out.add(("lm_head", nt, nx, -1, rec["head_fpt"], 0, 1 if backward else 0, -1))
    return out


def program_on_cpu(spec):
    """The descriptor of a network (no tensors are read by the plan query)."""
    import torch

    import oracle as O
    from hip_helpers import program_from_spec

    prog, _ = program_from_spec(spec, O.init_state_dict(spec, seed=0), torch.device("cpu"))
    prog.set_layer_major(True)
    return prog


def planned_matrix():
    """Every variant the plans of the whole network list hold, under this process's policy."""
    import os

    policy = policy_of_env(os.environ)
    out = set()
    for nt, nx, fam in cases():
        for label, spec in networks(nt, nx, fam):
            fwd, bwd = network_variants(label, spec, nt, nx, fam, policy)
            out |= fwd | bwd
    return out


def policy_of_env(env):
    if env.get("PINN_LM_FUSED") == "0":
        return "unfused"
    if env.get("PINN_LM_FUSED_LN") == "15":
        return "all_ln_fused"
    assert "PINN_LM_FUSED" not in env and "PINN_LM_FUSED_LN" not in env, "a policy this matrix does not enumerate"
    return "default"


# ---- the matrix, by enumeration ------------------------------------------------------------------------------------------
SHAPES = [(4, 4), (4, 8), (8, 8)]  # (nch, rt): depth 128 x 128 rows, depth 128 x 256-row blocks, depth 256 x 256-row blocks
FPTS = [1, 4, 8, 16]
SIN = FAM_ID["sin"]


def instantiated():
    """Every instantiation lm_fused_inst.hip and lm_inst.hip hold for the stream sets of this matrix (without the XG forms
    of the reverse element-wise kernels), as variants; lm_head, one template per FPT, counts once per launch mode."""
    out = set()
    for nt, nx in FUSED_SETS:
        out |= {("lm_fused", nt, nx, f, sh, ln, b, aux) for f in range(5) for sh in SHAPES for ln in (0, 1) for b in (0, 1) for aux in (0, 1)}
    for nt, nx in SETS:
        out |= {("lm_ew", nt, nx, f, fpt, ln, b, 0) for f in range(5) for fpt in FPTS for ln in (0, 1) for b in (0, 1)}
        out |= {("lm_ew", nt, nx, f, 4, 1, 1, 1) for f in range(5)}  # lm_ew_bwd_dma: LayerNorm, FPT 4
        out |= {("lm_fourier_fwd", nt, nx, -1, fpt, 0, 0, 2) for fpt in FPTS}
        out |= {("lm_head", nt, nx, -1, fpt, 0, b, -1) for fpt in FPTS for b in (0, 1)}
    return out


def unreachable_reason(v):
    """Why no descriptor of a reference architecture reaches an instantiated variant (None: it is reachable)."""
    kern, nt, nx, fam, shape, ln, bwd, last = v
    if kern in ("lm_fused", "lm_ew") and fam == SIN and ln:
        # lm_engine.hip::build_program: `const bool ln = d->arch == PINN_ARCH_FEEDFORWARD && ...` — SIREN, whose activation
        # is sin, takes no LayerNorm, and no reference architecture offers sin as a feedforward / ResNet activation
        # (oracle `_act`).  Only a hand-made descriptor (feedforward + PINN_ACT_SIN + PINN_FLAG_LAYER_NORM) gets there.
        return "sin with LayerNorm: SIREN has no LayerNorm and no other reference architecture has sin"
    if kern == "lm_fused" and last and not ln:
        # AUX needs a skip record (ResNet: `pro.skip_node = n1` always with `pro.ln_g = base + 6`) or an add record
        # (attention: both adding nodes feed `p1.ln_g = base + 8` / `pro.ln_g = base + 14`; in reverse the records with an
        # extra cotangent are V of ResNet's n1 (LayerNorm + skip prologue from block 2 on; the first block's is fed by the
        # coordinates and never fused: plan_fusion `pro.src_kind == SRC_REC`), V of attention's merged node (LayerNorm
        # prologue, same remark) and V of its n1 (LayerNorm prologue): build_program
        return "AUX without LayerNorm: every skip / add record meets a LayerNorm prologue"
    if kern == "lm_fused" and last and shape == (4, 8):
        # AUX nodes are H -> H (ResNet, attention's merged node) or the FFN's H -> 4 H -> H; (4, 8) is 256 rows at depth 128:
        # fuse_shape on (4 H = 256, H = 64) / (64, 256) refuses rows 64 (`rp == 128 && dp == 128`, `rp % 256 == 0`)
        return "AUX at 256 rows x depth 128: no skip / add node has that shape"
    return None


def reachable(policy="all_ln_fused"):
    """The reachable matrix, under a policy: "all_ln_fused" (PINN_LM_FUSED_LN=15) plans every reachable fused variant and
    is the matrix; "default" leaves the LayerNorm reverse epilogues at depth 256 to GEMM + lm_ew_bwd(_dma)
    (lm_engine.hip::fused_ln_mask, bit 8); "unfused" (PINN_LM_FUSED=0) plans no fused kernel.  The element-wise, Fourier
    and head variants are planned under every policy (nodes fuse_shape refuses, first prologues, heads, time order 2)."""
    out = {v for v in instantiated() if unreachable_reason(v) is None}
    if policy == "unfused":
        out = {v for v in out if v[0] != "lm_fused"}
    elif policy == "default":
        out = {v for v in out if not (v[0] == "lm_fused" and v[5] and v[6] and v[4] == (8, 8))}
    else:
        assert policy == "all_ln_fused", policy
    return out


def fpt_of(features):
    """Features per thread of an element-wise launch (lm_engine.hip::fpt_for) — used for the SUBJECT of a case only: the
    plan, not this function, says what runs."""
    hp = (features + 31) // 32 * 32
    return 1 if hp <= 64 else (4 if hp <= 256 else (8 if hp <= 512 else 16))


def subject(label, spec, nt, nx, fam, policy):
    """The variants a network is in the list FOR (a subset of what it plans): the GPU case asserts that its plan holds
    them, so that a policy change cannot silently turn the case into a test of something else."""
    f = FAM_ID[fam]
    K = 1 + nt + nx
    fused = (nt, nx) in FUSED_SETS and policy != "unfused"
    deep_ln = policy == "all_ln_fused"  # LayerNorm reverse epilogues at depth 256
    s = set()
    if label == "A":
        s |= {("lm_ew", nt, nx, f, 4, 0, b, 0) for b in (0, 1)}  # the first Linear's prologue
        if fused:
            s |= {("lm_fused", nt, nx, f, sh, 0, b, 0) for sh in SHAPES for b in (0, 1)}
    elif label == "B":
        s |= {("lm_ew", nt, nx, f, 4, 1, b, 0) for b in (0, 1)}  # first prologue forward; the head's adjoint has no LDS-DMA form
        if fused:
            s |= {("lm_fused", nt, nx, f, sh, 1, 0, 0) for sh in SHAPES}
            s |= {("lm_fused", nt, nx, f, sh, 1, 1, 0) for sh in ((4, 4), (4, 8))}
            s.add(("lm_fused", nt, nx, f, (8, 8), 1, 1, 0) if deep_ln else ("lm_ew", nt, nx, f, 4, 1, 1, 1 if K * 256 <= 1024 else 0))
        else:
            s.add(("lm_ew", nt, nx, f, 4, 1, 1, 1))  # width 128: K * Hp <= 1024 for every stream set
    elif label in ("C", "C_ln"):
        ln = 1 if label == "C_ln" else 0
        s |= {("lm_ew", nt, nx, f, fpt, ln, b, 0) for fpt in (1, 8, 16) for b in (0, 1)}
        s |= {("lm_head", nt, nx, -1, fpt_of(spec.dims()[-1]), 0, b, -1) for b in (0, 1)}
    elif label == "F":
        s.add(("lm_fourier_fwd", nt, nx, -1, fpt_of(2 * spec.mapping_size), 0, 0, 2))
        s |= {("lm_head", nt, nx, -1, 4, 0, b, -1) for b in (0, 1)}
    elif label[0] == "R" and fused:
        sh = (4, 4) if spec.hidden_dim == 128 else (8, 8)
        s |= {("lm_fused", nt, nx, f, sh, 1, 0, aux) for aux in (0, 1)}
        if sh == (4, 4) or deep_ln:
            s |= {("lm_fused", nt, nx, f, sh, 1, 1, aux) for aux in (0, 1)}
    elif label[0] == "R":
        s.add(("lm_ew", nt, nx, f, 4, 1, 1, 0))  # the head's skip prologue: its adjoint has no LDS-DMA form
        if K * spec.hidden_dim <= 1024:
            s.add(("lm_ew", nt, nx, f, 4, 1, 1, 1))  # the skip prologue of the second block
    elif label[0] == "T" and fused:
        sh = (4, 4) if spec.hidden_dim == 128 else (8, 8)
        relu, gelu = FAM_ID["relu"], FAM_ID["gelu"]
        s.add(("lm_fused", nt, nx, relu, sh, 1, 0, 1))  # an add record in front of a LayerNorm without activation
        s.add(("lm_fused", nt, nx, gelu, (sh[0], 8), 0, 0, 0))  # H -> 4 H: two / four 256-row blocks
        if sh == (4, 4) or deep_ln:
            s.add(("lm_fused", nt, nx, relu, sh, 1, 1, 1))
    return s


def network_variants(label, spec, nt, nx, fam, policy, n=N_PTS):
    """(forward variants, reverse variants) of one network's plans; asserts the layer-major engine runs, the plan stays
    inside the matrix and holds the network's subject."""
    from pinnrl_amd import _lib

    prog = program_on_cpu(spec)
    out = []
    for bwd in (0, 1):
        assert _lib.kernel_for(prog, n, nt, nx, bwd)["engine"] == "layer_major", (label, nt, nx, bwd)
        out.append(plan_variants(_lib.lm_plan(prog, n, nt, nx, bwd), nt, nx, bwd))
    both = out[0] | out[1]
    assert both <= reachable(policy), (label, nt, nx, fam, sorted(both - reachable(policy)))
    missing = subject(label, spec, nt, nx, fam, policy) - both
    assert not missing, f"({nt},{nx}) {fam} {label} under {policy}: not planned: {sorted(missing)}"
    return out
