"""Rank-based pruning of kNN lists on the host (hipzap/search.py): ``graph_prune_ref`` on lists whose detour counts
can be written down, the options that reach it, and what it does to the recall of the reference walk."""
import numpy as np
import pytest

from hipzap import _native as N
from hipzap import search as S
from hipzap.__main__ import main as cli

W = 16


def lists(offsets, n=12):
    """Row x holds (x + o) % n for each offset, then -1 up to W."""
    knn = np.full((n, W), -1, np.int32)
    knn[:, :len(offsets)] = (np.arange(n)[:, None] + np.array(offsets)) % n
    return knn


def ring():
    """Row x = [x+1, x-1, x+2, x-2, x+6]: x+2 is knn[x+1][0] and x-2 is knn[x-1][1], one detour each over better-ranked
    edges; the chord x+6 is in no neighbour's first four columns and moves ahead of them."""
    det = np.zeros((12, W), np.int32)
    det[:, 2:4] = 1
    return lists([1, -1, 2, -2, 6]), lists([1, -1, 6, 2, -2]), det


def no_detours():
    """Row x = [x+1, x+3] (knn[x+1][0] is x+2): the order is the list. Row 0 holds only itself, padding and ids outside
    [0, N): all -1."""
    knn = lists([1, 3])
    knn[0, :6] = [0, -1, 12, -5, 0, 99]
    return knn, np.where(np.arange(12)[:, None] == 0, -1, knn), np.zeros((12, W), np.int32)


def invalid_columns():
    """The ring with row 5 = [6, 5 (itself), 4, 15 (outside), 6 (repeated), 7, 3, 11]: 7 is knn[6][0] and 3 is knn[4][1],
    one detour each; 4 and 11 have none. Only row 5 is stated."""
    knn = ring()[0]
    knn[5, :8] = [6, 5, 4, 15, 6, 7, 3, 11]
    return knn, np.array([6, 4, 11, 7, 3] + [-1] * 11), np.array([0] * 5 + [1, 1] + [0] * 9)


@pytest.mark.parametrize("case,rows", [(ring, slice(None)), (no_detours, slice(None)), (invalid_columns, 5)])
def test_hand_counted_lists(case, rows):
    knn, order, det = case()
    got_order, got_det = S.graph_prune_ref(knn)
    assert got_order.dtype == np.int32 == got_det.dtype and got_order.shape == knn.shape == got_det.shape
    assert np.array_equal(got_order[rows], order) and np.array_equal(got_det[rows], det)
    assert np.array_equal(S.graph_prune(knn), got_order) and N.KINDS["HZ_K_GRAPH_PRUNE"] == 57
    for bad in (knn[:, :12], knn[:, :8], knn.astype(np.float32), np.zeros((4, 136), np.int32)):
        with pytest.raises(ValueError, match="knn must be"):
            S.graph_prune(bad)


N_ROWS, DIM, DEG, NQ = 2048, 64, 16, 64


@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    """Overlapping clusters: 64 unit-variance centres, noise 1.0, cosine; the queries are stored rows with noise added."""
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((64, DIM)).astype(np.float32)
    rows = cent[rng.integers(0, 64, N_ROWS)] + rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    q = rows[rng.choice(N_ROWS, NQ, replace=False)] + 0.5 * rng.standard_normal((NQ, DIM)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("p") / "c.hzidx")
    S.write_index(path, rows, "cosine")
    return path, rows, q


def recall(ids, truth):
    return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids, truth)) / truth.size


def test_pruning_raises_the_recall_of_the_reference_walk(clustered):
    """Recall@10 of ``search_graph_ref`` (beam 32, width 1, iters 128, 64 entry rows) over 64 queries, measured on the
    CPU at N = 2,048 (4,096 took 13 s, nearly all of it the fp64 kNN lists): 0.766 on the kNN graph of degree 16, 1.000
    on the pruned one (lists of width 32); at N = 4,096 they were 0.702 and 0.859. The walk is deterministic; the margin
    of half that gap covers another draw of queries."""
    path, rows, q = clustered
    with S.RefIndex(path) as ref:
        truth = ref.search(q, 10)[1]
        knn = ref.knn_graph(2 * DEG)[0]
        plain = S.graph_build(knn[:, :DEG], DEG)  # a list's first half is the list of half the width
        ref.set_graph(plain)
        r_plain = recall(ref.search_graph(q, 10, beam=32, width=1, iters=128)[1], truth)
        pruned = ref.build_graph(DEG, prune=True)
        r_pruned = recall(ref.search_graph(q, 10, beam=32, width=1, iters=128)[1], truth)
    print("recall@10: kNN graph", r_plain, "pruned", r_pruned)
    assert r_pruned - r_plain >= (1.000 - 0.766) / 2
    assert np.array_equal(pruned, S.graph_build(S.graph_prune_ref(knn)[0], DEG)) and not np.array_equal(pruned, plain)


def test_the_options_that_reach_it(clustered, tmp_path):
    path, rows, _ = clustered
    small, vec, a, b = rows[:200], str(tmp_path / "v.npy"), str(tmp_path / "a.hzidx"), str(tmp_path / "b.hzidx")
    np.save(vec, small)
    for call in (lambda: S.write_index(a, small, "cosine", graph_prune=True),
                 lambda: S.convert_index(path, a, "bf16", graph_prune=True)):
        with pytest.raises(ValueError, match="graph_prune goes with graph=DEG"):
            call()
    with pytest.raises(SystemExit, match="--graph-prune goes with --graph"):
        cli(["index", "--vectors", vec, "--out", a, "--graph-prune"])
    S.write_index(a, small, "cosine", graph=8, graph_prune=True)
    cli(["index", "--vectors", vec, "--out", b, "--metric", "cosine", "--graph", "8", "--graph-prune"])
    assert S.file_info(a)["version"] == 12 and open(a, "rb").read() == open(b, "rb").read()
    S.write_index(b, small, "cosine")
    with S.RefIndex(b) as ref:
        assert np.array_equal(S.read_graph(a)[0], ref.build_graph(8, prune=True))
