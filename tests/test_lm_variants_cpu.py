"""CPU test (no GPU): the network list of the layer-major variant matrix (tests/lm_variants_model.py) plans every
reachable variant of the layer-major kernels, as `pinn_lm_plan` reports them — the query answers from the functions
lm_run launches from (plan_fusion, fused_set_built, fpt_for, lm_fused_aux, lm_ew_bwd_dma_shape), so a policy change that
would empty a GPU case of its subject fails here first.  The policy is read once per process: the default policy is
checked in this process, PINN_LM_FUSED=0 and PINN_LM_FUSED_LN=15 in child processes.

The matrix (lm_variants_model.reachable / instantiated / unreachable_reason), by enumeration:
  lm_fused    6 stream sets x 5 families x 3 shapes x LN x BWD x AUX = 720 instantiated, 420 reachable: without LayerNorm
              3 shapes x 2 directions x 5 families = 30 per set; with LayerNorm the 4 families other than sin x 2 directions
              x ((4, 4) and (8, 8) with and without AUX, (4, 8) without) = 40 per set.  Unreachable per set: AUX without
              LayerNorm (30), sin with LayerNorm (12), AUX at (4, 8) with LayerNorm (8).
  lm_ew       8 stream sets x (5 families x 4 FPT x LN x {lm_ew_fwd, lm_ew_bwd} + 5 lm_ew_bwd_dma) = 680 instantiated, 608
              reachable: sin with LayerNorm (8 + 1 per set) is not.
  lm_fourier_fwd   8 x 4 FPT = 32;   lm_head   8 x 4 FPT, forward-only and reverse launches = 64.
1 124 reachable variants of 1 496; the default policy plans 1 076 (not the 48 LayerNorm reverse epilogues at depth 256),
the unfused policy the 704 that are not lm_fused.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import lm_variants_model as M
print("PLANNED " + json.dumps(sorted(map(repr, M.planned_matrix()))))
"""


def _planned(policy):
    import lm_variants_model as M

    if policy == "default":
        assert M.policy_of_env(os.environ) == "default", "run this test without PINN_LM_FUSED / PINN_LM_FUSED_LN set"
        return M.planned_matrix()
    env = {k: v for k, v in os.environ.items() if k not in ("PINN_LM_FUSED", "PINN_LM_FUSED_LN")}
    env.update(M.POLICIES[policy])
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("PLANNED ")][-1]
    return {eval(v) for v in json.loads(line[len("PLANNED "):])}  # reprs of tuples of ints and strings


def test_matrix_enumeration():
    """The enumeration adds up, and every instantiated variant is reachable or excluded by a stated line of the engine."""
    import lm_variants_model as M

    inst, reach = M.instantiated(), M.reachable()
    count = lambda s, k: sum(1 for v in s if v[0] == k)
    assert (count(inst, "lm_fused"), count(inst, "lm_ew")) == (720, 680) and len(inst) == 1496
    assert (count(reach, "lm_fused"), count(reach, "lm_ew"), count(reach, "lm_fourier_fwd"), count(reach, "lm_head")) == (420, 608, 32, 64)
    assert len(reach) == 1124 and reach <= inst
    reasons = {}
    for v in inst - reach:
        why = M.unreachable_reason(v)
        assert why, v
        reasons[why] = reasons.get(why, 0) + 1
    assert sorted(reasons.values()) == [48, 144, 180] and sum(reasons.values()) == 372, reasons
    assert len(M.reachable("default")) == 1076 and len(M.reachable("unfused")) == 704
    assert M.reachable("default") | M.reachable("unfused") <= reach


_PLANNED = {}


@pytest.mark.parametrize("policy", ["default", "unfused", "all_ln_fused"])
def test_network_list_plans_the_reachable_matrix(policy):
    import lm_variants_model as M

    planned = _planned(policy)
    _PLANNED[policy] = planned
    want = M.reachable(policy)
    assert planned == want, (f"{policy}: planned but not in the matrix {sorted(planned - want)[:10]}, "
                             f"in the matrix but not planned {sorted(want - planned)[:10]}")


def test_every_reachable_variant_is_planned():
    """Runs after the three policies (file order): their union is the matrix."""
    import lm_variants_model as M

    assert set(_PLANNED) == set(M.POLICIES), "the policy cases did not all run"
    union, full = set().union(*_PLANNED.values()), M.reachable()
    print(f"{len(union & full)} of {len(full)} reachable layer-major variants planned "
          f"(default {len(_PLANNED['default'])}, unfused {len(_PLANNED['unfused'])}, all LayerNorm nodes fused {len(_PLANNED['all_ln_fused'])}; "
          f"{len(M.instantiated()) - len(full)} instantiated variants are unreachable, lm_variants_model.unreachable_reason)")
    assert union == full


def test_plan_records_of_a_known_network():
    """The plan of one network, field by field: ResNet 2 x 128 on Burgers' streams, reverse."""
    import oracle as O
    import lm_variants_model as M
    from pinnrl_amd import _lib

    prog = M.program_on_cpu(O.ArchSpec("resnet", hidden_dim=128, num_layers=2, num_blocks=2, activation="tanh"))
    plan = _lib.lm_plan(prog, 100, 1, 2, 1)
    assert len(plan) == 5  # four GEMM nodes and the head
    first, n2, n1b, head = plan[0], plan[1], plan[2], plan[4]
    assert (first["src_kind"], first["fwd_fused"], first["fwd_ew_kind"], first["fwd_fpt"], first["bwd_ew_kind"]) == (1, 0, 0, 4, 0)
    assert (n2["has_ln"], n2["has_skip"], n2["fwd_fused"], n2["fwd_aux"], n2["bwd_fused"], n2["bwd_aux"]) == (1, 0, 1, 0, 1, 0)
    assert (n2["fwd_nch"], n2["fwd_rt"], n2["fwd_gy"], n2["rows"], n2["depth"], n2["act_family"]) == (4, 4, 1, 128, 128, 0)
    assert (n1b["has_skip"], n1b["fwd_fused"], n1b["fwd_aux"], n1b["bwd_fused"], n1b["bwd_aux"]) == (1, 1, 1, 1, 1)
    assert (head["has_skip"], head["fwd_fused"], head["fwd_aux"], head["bwd_fused"], head["bwd_ew_kind"], head["head_fpt"]) == (1, 1, 1, 0, 0, 4)
    fwd_only = _lib.lm_plan(prog, 100, 1, 2, 0)
    assert all(r["bwd_fused"] == 0 and r["bwd_ew_kind"] == -1 for r in fwd_only)
    assert [r["fwd_fused"] for r in fwd_only] == [r["fwd_fused"] for r in plan]
    # a stream set without fused units, and the statuses of pinn_kernel_for
    assert all(r["fwd_fused"] == 0 and r["bwd_fused"] == 0 for r in _lib.lm_plan(prog, 100, 2, 2, 1))
    with pytest.raises(ValueError):
        _lib.lm_plan(prog, 100, 3, 0, 1)
    lib = _lib.load()
    import ctypes

    recs = (_lib.PinnLmNodePlan * 2)()
    assert lib.pinn_lm_plan(ctypes.byref(prog.desc), 100, 1, 2, 1, recs, 2) == -1  # too few records: PINN_ERR_BAD_DESC
    assert lib.pinn_abi_version() == 2 == _lib.PINN_ABI_VERSION  # the change is additive
