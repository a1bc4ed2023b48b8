"""The batch scans' merged results bit for bit against tests/golden/batch_bits.npz, recorded on an MI355X from the
build before the three batch-scan kernels (MSCAN, XSCAN, PQXSCAN) were stated once over shared pieces
(scripts/batch_bits_record.py): the u32 view of every score and every id (tests/batch_bits_cases.py). The existing
suites compare kernels of one build with each other and with fp64 oracles; this one pins them to an earlier build."""
import os

import numpy as np
import pytest

import batch_bits_cases as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_the_recipe_is_unambiguous_and_the_fixture_holds_the_oracles_ids(golden):
    """Host only: every case's fp64 top-k is forced under twice the error bound over its passing rows, no two of the
    top k + 1 scores are equal, every query with a passing row gets k distinct real rows (none degenerates to
    sentinels), the recorded ids are the oracle's and the recorded scores lie within the bound of the fp64 scores."""
    assert sorted(golden) == sorted([n + "_ids" for n in B.NAMES] + [n + "_scores" for n in B.NAMES])
    assert not B.LIVE[16:32].any() and not B.LIVE[64:128].any() and 0 < (~B.LIVE[32:48]).sum() < 16 and B.LIVE[256:].all()
    for name, kind, D, arg, Q, k, salt in B.CASES:
        inp = B.inputs(name)
        s, b, allow = B.oracle(name, inp)
        assert (inp["bits"][B.NAN_ROW] == 0x7FC0).all() and np.isfinite(S_rows(inp)[B.LIVE]).all(), name
        want = B.ref_ids(name, inp)
        void = ~allow.any(axis=1)
        assert void.sum() == (1 if kind == "mscan" and Q >= 17 else 0), name
        for qi in np.flatnonzero(~void):
            assert (want[qi] >= 0).all() and np.unique(want[qi]).size == k and allow[qi][want[qi]].all(), name
        assert (want[void] == -1).all()
        ids = golden[name + "_ids"]
        if k == 10:  # the order is forced: the recorded ids are the oracle's
            assert B.subset_ambiguous(s, b, k, allow) == 0, name
            for qi in np.flatnonzero(~void):
                top = np.sort(s[qi][allow[qi]])[::-1][:k + 1]
                assert top.size > k and np.unique(top).size == top.size, name
            assert np.array_equal(ids, want), name
        else:  # k = 128: k distinct passing rows per query
            assert all(np.unique(r).size == k and allow[qi][r].all() for qi, r in enumerate(ids)), name
        got = golden[name + "_scores"].view(np.float32).astype(np.float64)
        rows = np.flatnonzero(~void)[:, None]
        assert (np.abs(got[~void] - s[rows, ids[~void]]) <= b[rows, ids[~void]]).all(), name
        assert (got[void] == -np.inf).all(), name


def S_rows(inp):
    from hipzap import search as S
    return S.bf16_to_f32(inp["bits"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", B.NAMES)
def test_scores_and_ids_equal_the_recorded_bits(name, golden):
    bits, ids = B.run_case(name)
    assert np.array_equal(ids, golden[name + "_ids"]), name
    assert np.array_equal(bits, golden[name + "_scores"]), (name, bits ^ golden[name + "_scores"])
