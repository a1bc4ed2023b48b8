"""The scan kernels' results bit for bit against tests/golden/search_bits.npz, recorded on an MI355X from the build
before the three scan kernels became one template (scripts/search_bits_record.py): the u32 view of every score
and every id, one case per instantiation (tests/search_bits_cases.py). The existing suites compare kernels of
one build with each other; this one pins them to an earlier build."""
import os

import numpy as np
import pytest

import search_bits_cases as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_the_recipe_is_unambiguous_and_the_fixture_holds_the_oracles_ids(golden):
    """Host only: every case's fp64 top-k is forced under twice the fp32 bound over its passing rows, no two of
    the top k + 1 scores are equal, the recorded ids are ``search_ref``'s and the recorded scores lie within the
    fp32 bound of the fp64 scores."""
    assert sorted(golden) == sorted([n + "_ids" for n in B.NAMES] + [n + "_scores" for n in B.NAMES])
    for name, kind, D, salt in B.CASES:
        inp = B.inputs(kind, D, salt)
        s, b = B.oracle(inp)
        assert B.subset_ambiguous(s, b, B.K, inp["allow"]) == 0, name
        for qi in range(B.Q):
            top = np.sort(s[qi][inp["allow"][qi]])[::-1][:B.K + 1]
            assert top.size > B.K and np.unique(top).size == top.size, name
        assert not np.isnan(inp["rows32"]).any() and np.isfinite(inp["rows32"]).all() and np.isfinite(inp["q"]).all()
        if kind != "scan":
            assert not inp["live"][8:12].any() and 0 < (~inp["live"]).sum() < B.N // 2
            assert len({inp["allow"][qi].tobytes() for qi in range(B.Q)}) == B.Q  # another subset per query
        if kind == "qscan":
            assert (np.frexp(inp["scales"])[0] != 0.5).all()  # no power of two
        ids = golden[name + "_ids"]
        assert np.array_equal(ids, B.ref_ids(inp)), name
        got = golden[name + "_scores"].view(np.float32).astype(np.float64)  # the recorded scores are the oracle's
        rows = np.arange(B.Q)[:, None]
        assert (np.abs(got - s[rows, ids]) <= b[rows, ids]).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", B.NAMES)
def test_scores_and_ids_equal_the_recorded_bits(name, golden):
    bits, ids = B.run_case(name)
    assert np.array_equal(ids, golden[name + "_ids"]), name
    assert np.array_equal(bits, golden[name + "_scores"]), (name, bits ^ golden[name + "_scores"])
