"""``.hzidx`` version 12 on the GPU (csrc/index.cpp: hz_index_open*, hz_index_set_graph, hz_index_search_graph):
``Index.search_graph`` against ``RefIndex`` and ``Index.search``."""
import numpy as np
import pytest

from hipzap import search as S

pytestmark = pytest.mark.gpu
N_ROWS, DIM, NQ = 4096, 64, 64
BEAM, WIDTH = 64, 1
NOISE = 1.0  # of unit-variance centres: the clusters overlap (tight ones split a kNN graph into components)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clustered():
    rng = np.random.default_rng(11)
    cent = rng.standard_normal((64, DIM)).astype(np.float32)
    rows = cent[rng.integers(0, 64, N_ROWS)] + NOISE * rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    q = cent[rng.integers(0, 64, NQ)] + NOISE * rng.standard_normal((NQ, DIM)).astype(np.float32)
    return rows, q


def recall(ids, truth):
    return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids, truth)) / truth.size


def test_a_version_12_index_against_the_reference_walk_and_the_plain_index(tmp_path):
    """Recall@10 over 64 queries against ``RefIndex.search``, beam 64, width 1, ``write_index(graph=32)``: the reference
    walk's own recall, computed on the CPU, is 0.967 (>= 0.9 as required; beam 32 gives 0.889); the GPU's may be at most
    one point below it (an fp32 / fp64 near-tie in the beam costs a few of the 640 slots)."""
    rows, q = clustered()
    path, plain, again = (str(tmp_path / n) for n in ("g.hzidx", "p.hzidx", "s.hzidx"))
    hdr = S.write_index(path, rows, "cosine", graph=32, graph_backend="gpu")
    S.write_index(plain, rows, "cosine")
    with S.Index(path) as ix, S.RefIndex(path) as ref, S.Index(plain) as px:
        assert ix.version == 12 and ix.describe()["graph_deg"] == 32 == hdr["graph_deg"]
        truth = ref.search(q, 10)[1]
        ref_recall = recall(ref.search_graph(q, 10, beam=BEAM, width=WIDTH)[1], truth)
        assert ref_recall >= 0.9
        s, i, st = ix.search_graph(q, 10, beam=BEAM, width=WIDTH, stats=True)
        print("recall: reference walk", ref_recall, "gpu", recall(i, truth), "rows scored", st[:, 1].mean())
        assert recall(i, truth) >= ref_recall - 0.01
        assert (st[:, 1] < N_ROWS // 4).all() and (st[:, 0] >= 1).all()
        for lo, hi in ((0, NQ), (0, NQ), (5, 6)):  # the captured programs replay to the same answer
            rep = ix.search_graph(q[lo:hi], 10, beam=BEAM, width=WIDTH)
            assert np.array_equal(u32(rep[0]), u32(s[lo:hi])) and np.array_equal(rep[1], i[lo:hi])
        a, b = ix.search(q, 10), px.search(q, 10)  # the rows are a plain bf16 corpus
        assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])
        for call in (lambda: ix.add(rows[:1]), lambda: ix.delete([3]), lambda: ix.search(q, 10, filter=(0, 0))):
            with pytest.raises(ValueError, match="refused on an index with a graph"):
                call()
        with pytest.raises(ValueError, match="has none"):
            px.search_graph(q)
        ix.save(again)
    g0, g1 = S.read_graph(path), S.read_graph(again)
    assert np.array_equal(g0[0], g1[0]) and np.array_equal(g0[1], g1[1]) and open(path, "rb").read() == open(again, "rb").read()


def test_integer_rows_both_backends_and_an_attached_graph(tmp_path):
    rng = np.random.default_rng(12)
    rows = rng.integers(-3, 4, (600, 32)).astype(np.float32)
    q = rng.integers(-3, 4, (5, 32)).astype(np.float32)
    cpu, gpu, plain, fp8 = (str(tmp_path / n) for n in ("c.hzidx", "g.hzidx", "p.hzidx", "q.hzidx"))
    S.write_index(cpu, rows, "ip", graph=16)
    S.write_index(gpu, rows, "ip", graph=16, graph_backend="gpu")
    assert open(cpu, "rb").read() == open(gpu, "rb").read()  # exact integer scores: the same kNN lists, the same graph
    S.write_index(plain, rows, "ip")
    S.write_index(fp8, rows, "ip", dtype="fp8")
    graph = rng.integers(-1, 600, (600, 16)).astype(np.int32)
    with S.Index(plain) as ix, S.RefIndex(plain) as ref:
        ix.set_graph(graph)
        ref.set_graph(graph)
        for kw in (dict(beam=32, width=1), dict(beam=256, width=16, iters=20)):
            a, b = ix.search_graph(q, 10, stats=True, **kw), ref.search_graph(q, 10, stats=True, **kw)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), kw  # exact integer scores: the same walk
        with pytest.raises(ValueError, match="graph must"):
            ix.set_graph(graph[:, :12])
    with S.Index(fp8) as ix, pytest.raises(ValueError, match="plain bf16"):
        ix.set_graph(graph)
