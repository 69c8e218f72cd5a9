"""CPU: the case table of tests/test_gpu_rowchain.py (tests/kernel_edge_cases.py::ROWCHAIN_CASES) covers every edge of the
software-pipelined chained B row pass (csrc/rowchain.hip), and every k_rows_chain_* instantiation of the BUILT library is run by at
least one GPU case.  The tiling of mode 1 (csrc/api.hip, mcl_set_problem) and the stack signature (rowchain.hip, make_sig /
chain_signature) are restated here; a new signature or bucket without a case fails on a CPU."""
import os
import re
import sys

import pytest

from tests import kernel_edge_cases as kec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLS_ROWSEP, CLS_PF2, CLS_UNI, CLS_L2 = 0, 1, 2, 3
CLASS = {"nn": CLS_ROWSEP, "box": CLS_ROWSEP, "l1": CLS_ROWSEP, "parafac2": CLS_PF2, "unimodal": CLS_UNI, "l2ball": CLS_L2}


def make_sig(n, *cls):
    sig = n
    for k, c in enumerate(cls):
        sig |= c << (3 + 2 * k)
    return sig


SIG_ROWSEP, SIG_L2, SIG_UNI_L2 = make_sig(2, CLS_PF2, CLS_ROWSEP), make_sig(2, CLS_PF2, CLS_L2), make_sig(3, CLS_PF2, CLS_UNI, CLS_L2)
R64, NB2 = "R64", "NB2"


def signature(case):
    """chain_signature: 0 when the pipelined kernels do not serve the case, else the stack's signature"""
    r, stack = case["rank"], case["B"]
    nb = (r + 15) // 16
    if r % 4 or r < 4 or nb > 2 or case.get("inner_tol") or not 1 <= len(stack) <= 3:
        return 0
    if sum(d["kind"] == "l2ball" for d in stack) > 1:  # the chained pass carries one L2-ball slot (api.hip)
        return 0
    sig = make_sig(len(stack), *(CLASS[d["kind"]] for d in stack))
    return sig if sig in (SIG_ROWSEP, SIG_L2, SIG_UNI_L2) else 0


def bucket(case):
    return R64 if case["rank"] <= 16 else NB2


def tiles(J):
    """64-row tiles inside one slab: the row count of every tile, slab by slab"""
    return [[min(64, j - t) for t in range(0, j, 64)] for j in J]


CASES = {n: kec.ROWCHAIN_CASES[n] for n in kec.ROWCHAIN_CASES}
JS = {n: [int(j) for j in kec.rowchain_J(c)] for n, c in CASES.items()}


def test_every_case_is_served_by_the_chain():
    for n, c in CASES.items():
        assert signature(c), n
        assert min(JS[n]) >= c["rank"], (n, "a PARAFAC2 slab needs J_i >= rank")
        if c["rank"] >= 20:  # well-posed Y_i Delta^T (test_gpu_end_to_end.py, the c5_dims_stack note)
            assert min(JS[n]) >= 3 * c["rank"], n
    for n, c in kec.ROWCHAIN_OTHER_CASES.items():
        assert not signature(c), n


def test_signatures_buckets_and_ranks():
    have = {(signature(c), bucket(c)) for c in CASES.values()}
    assert have >= {(s, b) for s in (SIG_ROWSEP, SIG_L2, SIG_UNI_L2) for b in (R64, NB2)}, have
    assert {c["rank"] for c in CASES.values()} >= {4, 8, 12, 16, 20, 24, 28, 32}


def test_penalty_members():
    members = set()
    for c in CASES.values():
        for d in c["B"][1:]:
            members.add((d["kind"], bool(d.get("non_negativity", False))))
    assert members >= {("nn", False), ("box", False), ("l1", False), ("l1", True), ("l2ball", False), ("l2ball", True),
                       ("unimodal", False), ("unimodal", True)}, members
    assert any(c.get("constant_B") and c.get("l2B", 0.0) > 0 for c in CASES.values())
    assert {c["inner"] for c in CASES.values()} >= {1, 2, 5}


def test_tile_shapes():
    assert any(min(JS[n]) < 16 and 4 <= c["rank"] <= 12 for n, c in CASES.items())
    last_rows = {t[-1] for J in JS.values() for t in tiles(J)}
    assert last_rows >= {1, 15, 16, 17, 63, 64}, last_rows
    assert any(len(t) > 16 for J in JS.values() for t in tiles(J))  # a slab longer than 16 tiles
    n_tiles = {n: sum(len(t) for t in tiles(J)) for n, J in JS.items()}
    assert max(n_tiles.values()) > 64  # more tiles than sink slots
    assert {v % 4 for v in n_tiles.values()} == {0, 1, 2, 3}, n_tiles


def test_legs():
    for n in kec.ROWCHAIN_NB1_CASES:
        assert CASES[n]["rank"] <= 16
    assert {signature(CASES[n]) for n in kec.ROWCHAIN_NB1_CASES} == {SIG_ROWSEP, SIG_L2, SIG_UNI_L2}
    for legs in (kec.ROWCHAIN_NO_PASS_CHAIN_CASES, kec.ROWCHAIN_TRAJECTORY_CASES):
        assert {(signature(CASES[n]), bucket(CASES[n])) for n in legs} == {(s, b) for s in (SIG_ROWSEP, SIG_L2, SIG_UNI_L2)
                                                                            for b in (R64, NB2)}
    assert min(kec.ROWCHAIN_NO_PASS_CHAIN_CASES.values()) >= 3


def claimed_instantiations():
    """k_rows_chain_{first,mid,last}<NBR, R64, SIG> that the GPU cases launch (mid: inner_n_iter_max >= 2 with the chain on)"""
    out = set()

    def claim(c, nbr, r64, inner):
        forms = ["first", "last"] + (["mid"] if inner >= 2 else [])
        out.update(f"k_rows_chain_{f}<{nbr}, {'true' if r64 else 'false'}, {signature(c)}>" for f in forms)

    for c in CASES.values():
        claim(c, 1 if c["rank"] <= 16 else 2, c["rank"] <= 16, c["inner"])
    for n in kec.ROWCHAIN_NB1_CASES:  # MCL_NO_ROWS64=1
        claim(CASES[n], 1, False, CASES[n]["inner"])
    return out


def test_every_chain_instantiation_has_a_case():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr

    if not os.path.exists(kr.LIB):
        pytest.skip(f"{kr.LIB} is not built (python -c 'import __graft_entry__ as g; g.build()')")
    built = {r["kernel"] for r in kr.resources() if re.match(r"k_rows_chain_(first|mid|last)<", r["kernel"])}
    assert len(built) >= 27, sorted(built)
    claimed = claimed_instantiations()
    assert not built - claimed, f"k_rows_chain_* instantiations no case of tests/kernel_edge_cases.py runs: {sorted(built - claimed)}"
    assert not claimed - built, f"cases claim instantiations the library does not have: {sorted(claimed - built)}"
