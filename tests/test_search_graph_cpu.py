"""The host side of the graph search (hipzap/search.py): ``graph_build``, ``.hzidx`` version 12, the CLI flag and
``RefIndex.search_graph`` (the numpy walk ``search_graph_ref``)."""
import json

import numpy as np
import pytest

from hipzap import _native as N
from hipzap import search as S
from hipzap.__main__ import main as cli


def test_graph_build_on_six_rows():
    """Hand-worked: row 0's list holds a padding entry, itself and a duplicate; the first halves are four ids; source 0
    gives row 5 the reverse edge 0, source 4 gives row 0 the edge 4, source 5 gives rows 1..4 the edge 5."""
    knn = np.full((6, 8), -1, np.int64)
    knn[0] = [5, -1, 0, 5, 1, 2, 3, 4]
    knn[1, :5], knn[2, :5], knn[3, :5] = [0, 2, 3, 4, 5], [0, 1, 3, 4, 5], [0, 1, 2, 4, 5]
    knn[4, :5], knn[5, :5] = [0, 1, 2, 3, 5], [1, 2, 3, 4, 0]
    g = S.graph_build(knn, 8)
    assert g.dtype == np.int32 and g.shape == (6, 8) and (g[:, 5:] == -1).all()
    assert g[:, :5].tolist() == [[5, 1, 2, 3, 4], [0, 2, 3, 4, 5], [0, 1, 3, 4, 5], [0, 1, 2, 4, 5], [0, 1, 2, 3, 5],
                                 [1, 2, 3, 4, 0]]
    for bad, word in (((knn, 12), "deg"), ((knn[:, :3], 8), "knn_ids")):
        with pytest.raises(ValueError, match=word):
            S.graph_build(*bad)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("g")
    rows = np.random.default_rng(0).integers(-3, 4, (40, 64)).astype(np.float32)
    np.save(d / "v.npy", rows)
    return d, rows, S.write_index(str(d / "g.hzidx"), rows, "ip", graph=16)


@pytest.mark.parametrize("old,new,word", [
    (b'"graph_deg": 16', b'"graph_deg": 12', "graph_deg"), (b'"entries": 40', b'"entries": 0 ', "entries"),
    (b'"graph_deg"', b'"graph_dex"', "without integers"), (b'"graph_off": 12288', b'"graph_off": 12289', "graph_off"),
    (b'"entries_off": 16384', b'"entries_off": 12288', "entries_off")])
def test_version_12_header_round_trip_and_malformed_keys(files, old, new, word):
    d, rows, hdr = files
    path = str(d / "g.hzidx")
    got = S.read_header(path)
    assert (hdr["graph_deg"], hdr["entries"]) == (16, 40) and all(got[k] == hdr[k] for k in S.GRAPH_KEYS)
    assert S.file_info(path)["version"] == 12 and hdr["graph_off"] % 4096 == 0 == hdr["entries_off"] % 4096
    graph, entries = S.read_graph(path)
    assert graph.shape == (40, 16) and entries.tolist() == list(range(40))
    assert np.array_equal(S.read_rows(path), S.read_rows(str(d / "g.hzidx"))) and np.array_equal(S.read_rows(path), S.to_bf16(rows))
    raw = open(path, "rb").read()
    assert raw.count(old) == 1
    bad = str(d / "bad.hzidx")
    open(bad, "wb").write(raw.replace(old, new))
    with pytest.raises(ValueError, match=word):
        S.read_header(bad)


def test_the_cli_flag_and_convert_index(files, capsys):
    d, rows, hdr = files
    out, conv, plain = str(d / "cli.hzidx"), str(d / "conv.hzidx"), str(d / "p.hzidx")
    cli(["index", "--vectors", str(d / "v.npy"), "--out", out, "--metric", "ip", "--graph", "16"])
    S.write_index(plain, rows, "ip")
    S.convert_index(plain, conv, "bf16", graph=16)
    want = open(str(d / "g.hzidx"), "rb").read()
    assert open(out, "rb").read() == want and open(conv, "rb").read() == want
    capsys.readouterr()
    cli(["info", out])
    assert json.loads(capsys.readouterr().out)["graph"]["graph_deg"] == 16
    with pytest.raises(SystemExit, match="graph"):
        cli(["index", "--vectors", str(d / "v.npy"), "--out", out, "--graph", "16", "--dtype", "fp8"])
    with pytest.raises(ValueError, match="graph"):
        S.write_index(out, rows, "ip", graph=16, tags=np.zeros(40, np.uint32))


def test_ref_index_search_graph_and_the_read_only_rule(files):
    d, rows, _ = files
    q = np.random.default_rng(1).integers(-3, 4, (3, 64)).astype(np.float32)
    graph = np.full((40, 64), -1, np.int32)
    for r in range(40):
        graph[r, :39] = np.delete(np.arange(40), r)
    with S.RefIndex(str(d / "p.hzidx")) as ref:
        with pytest.raises(ValueError, match="p.hzidx has none"):
            ref.search_graph(q)
        ref.set_graph(graph, [7])
        s, i, st = ref.search_graph(q, 64, stats=True)  # a complete graph: the exact search, then 24 empty slots
        es, ei = S.search_ref(rows, q, 40)
        assert s.dtype == np.float32 and np.array_equal(i[:, :40], ei) and np.array_equal(s[:, :40], es.astype(np.float32))
        assert (i[:, 40:] == -1).all() and (s[:, 40:] == -np.inf).all() and st.tolist() == [[40, 40]] * 3
        for kw, word in ((dict(beam=48), "beam"), (dict(k=65), "k must"), (dict(width=5), "width"), (dict(iters=0), "iters"),
                         (dict(iters=128), "iters")):
            with pytest.raises(ValueError, match=word):
                ref.search_graph(q, **{"k": 10, **kw})
    with S.RefIndex(str(d / "g.hzidx")) as ref:  # the file's own graph; and the index is read-only
        assert ref.version == 12 and ref.describe()["graph_deg"] == 16 and ref.search_graph(q, 5)[1].shape == (3, 5)
        for call in (lambda: ref.add(rows[:1]), lambda: ref.delete([3]), lambda: ref.set_tags([3], [1]),
                     lambda: ref.search(q, 5, filter=(0, 0)), lambda: ref.cluster(4)):
            with pytest.raises(ValueError, match="refused on an index with a graph"):
                call()
    assert N.KINDS["HZ_K_SEARCH_GRAPH"] == 56 and S.check_graph_args(10, 64, 1, None, 32, 64) == (10, 64, 1, 254)
