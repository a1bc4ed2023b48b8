"""The host side of per-query entry rows (hipzap/search.py): ``graph_seeds``, ``graph_seed_ref``, ``.hzidx``
version 13, the CLI flag, ``RefIndex.search_graph(seeds=)`` and what the seeds are worth on a clustered corpus."""
import hashlib

import numpy as np
import pytest

from hipzap import search as S
from hipzap.__main__ import main as cli


def clustered_case(seed=0, clusters=128, per=32, dim=64, nq=64):
    """128 tight clusters of 32 rows in random order (a degree-16 kNN graph falls apart into them) and queries near
    stored rows -> (fp32 rows [4096, 64], queries [64, 64])."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(rng.standard_normal((clusters, dim)), per, axis=0) + 0.1 * rng.standard_normal((clusters * per, dim))
    rows = rows[rng.permutation(rows.shape[0])].astype(np.float32)
    q = rows[rng.choice(rows.shape[0], nq, replace=False)] + 0.05 * rng.standard_normal((nq, dim)).astype(np.float32)
    return rows, q.astype(np.float32)


def recall(ids, truth):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / truth.shape[1] for a, b in zip(ids, truth)]))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("s")
    rows = np.random.default_rng(0).integers(-3, 4, (40, 64)).astype(np.float32)
    np.save(d / "v.npy", rows)
    return d, rows, S.write_index(str(d / "s.hzidx"), rows, "ip", graph=16, graph_seeds=24)


@pytest.mark.parametrize("old,new,word", [
    (b'"seeds": 24', b'"seeds": 0 ', "seeds 0"), (b'"seeds_off": 20480', b'"seeds_off": 20481', "seeds_off"),
    (b'"seeds_off": 20480', b'"seeds_off": 16384', "seeds_off"), (b'"seeds"', b'"seedz"', "without integers"),
    ((5).to_bytes(4, "little") + (6).to_bytes(4, "little"), (40).to_bytes(4, "little") + (6).to_bytes(4, "little"), "outside"),
    ((5).to_bytes(4, "little") + (6).to_bytes(4, "little"), (6).to_bytes(4, "little") * 2, "twice")])
def test_version_13_header_round_trip_and_malformed_keys(files, old, new, word):
    d, rows, hdr = files
    path = str(d / "s.hzidx")
    got = S.read_header(path)
    assert hdr["seeds"] == 24 and all(got[k] == hdr[k] for k in S.GRAPH_KEYS + S.SEED_KEYS) and hdr["seeds_off"] % 4096 == 0
    assert S.file_info(path)["version"] == 13 and S.file_info(path)["graph_seeds"] == 24
    seeds = S.read_seeds(path)
    assert np.array_equal(seeds, S.graph_seeds(40, 24)) and seeds[:4].tolist() == [0, 1, 3, 5] and S.graph_seeds(10, 64).size == 10
    raw = open(path, "rb").read()
    at = raw.find(old, 0 if old[:1] == b'"' else hdr["seeds_off"])  # an id pair: inside the seed block
    assert at >= 0 and (old[:1] != b'"' or raw.count(old) == 1)
    bad = str(d / "bad.hzidx")
    open(bad, "wb").write(raw[:at] + new + raw[at + len(old):])
    with pytest.raises(ValueError, match=word):
        S.read_header(bad)


V12_SHA256 = "5870b467c1b7f0d28ad302fcf7b9c4075251b5b5039a67cffe015c1cc889c8f9"  # the fixture's rows, graph=16, before version 13


def test_graph_alone_still_writes_its_version_12_bytes_and_seed_keys_belong_to_version_13(files):
    d, rows, hdr = files
    v12, v13 = str(d / "g12.hzidx"), str(d / "s.hzidx")
    S.write_index(v12, rows, "ip", graph=16)
    assert hashlib.sha256(open(v12, "rb").read()).hexdigest() == V12_SHA256 and S.file_info(v12)["version"] == 12
    raw = open(v13, "rb").read()
    open(str(d / "bad12.hzidx"), "wb").write(raw[:8] + (12).to_bytes(4, "little") + raw[12:])
    with pytest.raises(ValueError, match="belong to version 13"):
        S.read_header(str(d / "bad12.hzidx"))
    with pytest.raises(ValueError, match="no seed table"):
        S.read_seeds(v12)
    with S.RefIndex(v12) as ref, pytest.raises(ValueError, match="has none"):
        ref.search_graph(rows[:2], 5, seeds=4)


def test_the_cli_flag_and_convert_index_write_the_same_bytes(files):
    d, rows, hdr = files
    out, conv, plain = str(d / "cli.hzidx"), str(d / "conv.hzidx"), str(d / "p.hzidx")
    cli(["index", "--vectors", str(d / "v.npy"), "--out", out, "--metric", "ip", "--graph", "16", "--graph-seeds", "24"])
    S.write_index(plain, rows, "ip")
    S.convert_index(plain, conv, "bf16", graph=16, graph_seeds=24)
    want = open(str(d / "s.hzidx"), "rb").read()
    assert open(out, "rb").read() == want and open(conv, "rb").read() == want
    with pytest.raises(SystemExit, match="graph-seeds"):
        cli(["index", "--vectors", str(d / "v.npy"), "--out", out, "--graph-seeds", "24"])
    for kw in (dict(graph_seeds=24), dict(graph=16, graph_seeds=0), dict(graph=16, graph_seeds=8193)):
        with pytest.raises(ValueError, match="graph_seeds"):
            S.write_index(out, rows, "ip", **kw)


def test_ref_index_search_graph_with_seeds_and_its_refusals(files):
    d, rows, hdr = files
    q = np.random.default_rng(1).integers(-3, 4, (5, 64)).astype(np.float32)
    with S.RefIndex(str(d / "s.hzidx")) as ref:
        assert ref.version == 13 and ref.describe()["graph_seeds"] == 24
        ent = S.graph_seed_ref(ref._rows, q, ref.graph_seed_table, 4)
        score = q.astype(np.float64) @ ref._rows[ref.graph_seed_table].astype(np.float64).T
        assert all(ent[a].tolist() == ref.graph_seed_table[np.lexsort((np.arange(24), -score[a]))[:4]].tolist() for a in range(5))
        s, i, st = ref.search_graph(q, 5, beam=32, iters=3, seeds=4, stats=True)
        for a in range(5):
            es, ei, est = S.search_graph_ref(ref._rows, q[a:a + 1], ref.graph, ent[a], 5, 32, 1, 3)
            assert np.array_equal(i[a], ei[0]) and np.array_equal(s[a], es[0].astype(np.float32)) and np.array_equal(st[a], est[0])
        assert np.array_equal(ref.search_graph(q, 5, beam=32, iters=3)[1],
                              S.search_graph_ref(ref._rows, q, ref.graph, ref.graph_entries, 5, 32, 1, 3)[1])  # None: the shared entries
        for bad in (0, 65, 2.0):
            with pytest.raises(ValueError, match="seeds must be"):
                ref.search_graph(q, 5, seeds=bad)
        assert ref.save(str(d / "again.hzidx"))["seeds"] == 24
        assert open(str(d / "again.hzidx"), "rb").read() == open(str(d / "s.hzidx"), "rb").read()
        ref.set_graph(ref.graph, seeds=[7, 3, 39])  # an explicit table, e.g. medoids
        assert S.graph_seed_ref(ref._rows, q, [7, -1, 40, 3, 7], 8)[:, 3:].tolist() == [[-1] * 5] * 5
        for bad, word in (([3, 3], "twice"), ([40], "outside"), (np.zeros(0, np.int32), "1..8192")):
            with pytest.raises(ValueError, match=word):
                ref.set_graph(ref.graph, seeds=bad)


def test_per_query_entries_reach_the_querys_cluster_on_the_oracle(tmp_path):
    rows, q = clustered_case()
    path = str(tmp_path / "c.hzidx")
    S.write_index(path, rows, "cosine", graph=16, graph_seeds=512)
    with S.RefIndex(path) as ref:
        truth = ref.search(q, 10)[1]
        shared = recall(ref.search_graph(q, 10, beam=64, width=1, iters=64)[1], truth)
        seeded = recall(ref.search_graph(q, 10, beam=64, width=1, iters=64, seeds=16)[1], truth)
    print(f"recall@10: shared entries {shared:.3f}, seeds=16 of 512 {seeded:.3f}")
    assert seeded >= 0.95 and shared < 0.6
