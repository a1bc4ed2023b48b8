"""Binary indexes on the GPU (csrc/index.cpp over HZ_K_SEARCH_BSCAN): ``Index`` against ``RefIndex`` -- ids and
stage-one scores exactly --, the two-stage answers against the bf16 index bit for bit, the live scenario with 4m's
program rules, the by-name refusals from the native side and the routes. A few hundred rows, D = 128 and 768."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import search as S

import search_bin_cases as B
from search_bin_cases import T

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("D", [128, 768])
def test_index_equals_refindex_exactly_at_refine_0(tmp_path, D):
    rng = np.random.default_rng(D)
    v = rng.standard_normal((2 * T + 37, D)).astype(np.float32)
    v[T:T + 40] = v[:40]  # duplicated rows: ties across tiles
    q = (v[rng.integers(0, v.shape[0], 20)] + np.float32(0.7) * rng.standard_normal((20, D))).astype(np.float32)
    tags = (np.arange(v.shape[0]) % 7).astype(np.uint32)
    for rescore in (False, True):
        p = str(tmp_path / f"a{rescore}.hzidx")
        S.write_index(p, v, "cosine", dtype="bin", rescore=rescore, tags=tags)
        with S.Index(p, contexts=1) as ix, S.RefIndex(p) as ref:
            d = ix.describe()
            assert (d["dtype"], ix.version, d["backend"]) == ("bin_sign", 9 if rescore else 8, "gpu")
            for Q, k in ((1, 1), (3, 10), (16, 128), (20, 10)):  # 20: two native calls
                for kw in ({}, {"filter": (0xFFFFFFFF, 3)}, {"filter": [(1, 1)] * Q}):
                    got, want = ix.search(q[:Q], k, refine=0, **kw), ref.search(q[:Q], k, refine=0, **kw)
                    assert same(got, want), (Q, k, kw)
                    assert same(ix.search(q[:Q], k, refine=0, **kw), got)  # the captured program: the eager run's bits
            if not rescore:
                assert same(ix.search(q[:3], 10), ref.search(q[:3], 10))
                with pytest.raises(ValueError, match="refine must be None or 0.*bin_sign index of version 8"):
                    ix.search(q[:3], 10, refine=40)


@pytest.mark.parametrize("placement", ["device", "host"])
def test_two_stage_answers_are_the_bf16_indexes_bits(tmp_path, placement):
    # R covers every passing row: N <= 128, and a filter that passes <= 128 of 300
    rng = np.random.default_rng(9)
    for D, N, filt in ((128, 100, None), (768, 300, (0xFFFFFFFF, 2))):
        v = rng.standard_normal((N, D)).astype(np.float32)
        q = rng.standard_normal((5, D)).astype(np.float32)
        tags = (np.arange(N) % 3).astype(np.uint32)
        p9, p2 = str(tmp_path / f"n9_{D}.hzidx"), str(tmp_path / f"n2_{D}.hzidx")
        S.write_index(p9, v, "ip", dtype="bin", rescore=True, tags=tags)
        S.write_index(p2, v, "ip", tags=tags)
        with S.Index(p9, contexts=1, rescore_rows=placement) as ix, S.Index(p2, contexts=1) as bf:
            assert ix.describe()["rescore_rows"] == placement
            want = bf.search(q, 10, filter=filt)
            assert same(ix.search(q, 10, filter=filt, refine=128), want)
            assert same(ix.search(q, 10, filter=filt), want)  # None means 128
    # tight clusters: the sign bits alone give another answer, refine = 128 the bf16 answer bit for bit (the
    # precondition is asserted on the host, tests/test_search_bin_cpu.py)
    for D in (128, 768):
        v, q = B.clusters(D)
        qn = S.normalize_rows(q)
        p9, p1 = str(tmp_path / f"c9_{D}.hzidx"), str(tmp_path / f"c1_{D}.hzidx")
        S.write_index(p9, v, "cosine", dtype="bin", rescore=True)
        S.write_index(p1, v, "cosine")
        with S.Index(p9, contexts=1, rescore_rows=placement) as ix, S.Index(p1, contexts=1) as bf, S.RefIndex(p9) as ref:
            want = bf.search(qn, 10)
            assert not np.array_equal(ix.search(qn, 10, refine=0)[1], want[1])
            assert same(ix.search(qn, 10, refine=128), want)
            assert same(ix.search(qn, 10, refine=0), ref.search(qn, 10, refine=0))
    with S.Index(p9, contexts=1, rescore_rows="host") as a, S.Index(p9, contexts=1, rescore_rows="device") as b:
        v = S.read_rescore_rows(p9)  # the host placement keeps exactly the bf16 rows off the device
        assert b.describe()["device_bytes"] - a.describe()["device_bytes"] == b.describe()["capacity"] * v.shape[1] * 2


@pytest.mark.parametrize("rescore", [False, True])
def test_live_scenario_against_refindex_with_the_program_rules(tmp_path, rescore):
    D = 128
    A, Bv, q = B.index_data(D)
    A, pool = A[:200], np.concatenate([A[200:], Bv])  # 200 rows in the first tile, 356 to add
    path, saved = str(tmp_path / "a.hzidx"), str(tmp_path / "s.hzidx")
    S.write_index(path, A, "ip", dtype="bin", rescore=rescore)
    kw = {"refine": 0}
    with S.Index(path, contexts=1, reserve=2 * T) as ix, S.RefIndex(path, reserve=2 * T) as ref:
        def agree():
            for f in (None, (3, 1), [(0, 0), (0xFFFFFFFF, 9), (3, 2)]):
                assert same(ix.search(q, 10, filter=f, **kw), ref.search(q, 10, filter=f, **kw)), f
                if rescore:
                    assert np.array_equal(ix.search(q, 10, filter=f)[1], ref.search(q, 10, filter=f)[1]), f
        first = ix.search(q, 10, **kw)
        assert same(ix.search(q, 10, **kw), first) and ix.describe()["programs"] == 1
        for x in (ix, ref):
            assert list(x.add(pool[:8], tags=[1] * 8)) == list(range(200, 208))  # inside the first tile
        assert ix.describe()["programs"] == 1
        agree()
        n = ix.describe()["programs"]
        for x in (ix, ref):
            assert x.delete([3, 201]) == 2
            x.set_tags([10, 11], [9, 9])
        assert ix.describe()["programs"] == n  # deletes and tag writes change device data only
        agree()
        for x in (ix, ref):
            x.add(pool[8:108], tags=np.arange(100) % 4)  # across the tile boundary at T: the programs hold N
        assert ix.describe()["programs"] == 0 and ix.describe()["capacity"] == 2 * T
        agree()
        for x in (ix, ref):
            x.add(pool[108:])  # past the capacity of 2T: growth by doubling
        d = ix.describe()
        assert d["programs"] == 0 and d["capacity"] == 4 * T and d["count"] == B.IX_N + T and d["live"] == d["count"] - 2
        agree()
        words, tags, live, *rest = ix._state()
        rw, rt, rl, *rrest = ref._state()
        assert np.array_equal(words, rw) and np.array_equal(tags, rt) and np.array_equal(live, rl)
        if rescore:
            assert np.array_equal(rest[1], rrest[1])
        ix.save(saved)
        ref.save(str(tmp_path / "r.hzidx"))
        assert open(saved, "rb").read() == open(str(tmp_path / "r.hzidx"), "rb").read()
        want = ref.search(q, 10, **kw)
    with S.Index(saved, contexts=1) as again:
        assert again.version == (9 if rescore else 8) and same(again.search(q, 10, **kw), want)
        compact = str(tmp_path / "c.hzidx")
        assert again.save(compact, compact=True)["count"] == B.IX_N + T - 2
    with S.Index(compact, contexts=1) as ix, S.RefIndex(compact) as ref:
        assert same(ix.search(q, 10, **kw), ref.search(q, 10, **kw))


def test_by_name_refusals_from_the_native_side(tmp_path):
    v = np.random.default_rng(3).standard_normal((64, 128)).astype(np.float32)
    q = v[:2].copy()
    p8, p9 = str(tmp_path / "b8.hzidx"), str(tmp_path / "b9.hzidx")
    S.write_index(p8, v, "ip", dtype="bin")
    S.write_index(p9, v, "ip", dtype="bin", rescore=True)
    with S.Index(p8, contexts=1) as ix, S.Index(p9, contexts=1) as ix9:
        lib, h = ix._lib, ix._h
        err = lambda: lib.hz_index_last_error().decode()  # noqa: E731
        for call in (lambda: ix.neighbors([0], 3), lambda: ix.knn_graph(3), lambda: ix.cluster(2),
                     lambda: ix.search(q, 3, nprobe=2), lambda: ix.probes(q, 2)):
            with pytest.raises(ValueError, match="a bin_sign index of version 8"):
                call()
        out_s, out_i = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32)
        ids = np.zeros(1, np.int32)
        assert lib.hz_index_neighbors(h, 0, ids.ctypes.data, 1, 3, 1, out_s.ctypes.data, out_i.ctypes.data) == -35
        assert "a bin_sign index of version 8" in err()
        cent = np.zeros((2, 128), np.uint16)
        assert lib.hz_index_assign(h, 0, cent.ctypes.data, 2, None, out_i.ctypes.data, out_s.ctypes.data) == -38
        assert "a bin_sign index of version 8" in err()
        assert lib.hz_index_search3(h, 0, q.ctypes.data, None, 2, 3, 0, 2, out_s.ctypes.data, out_i.ctypes.data) == -34
        assert "bin_sign index of version 8" in err()
        assert lib.hz_index_probes(h, 0, q.ctypes.data, 2, 2, out_i.ctypes.data) == -34 and "bin_sign" in err()
        assert lib.hz_index_search3(h, 0, q.ctypes.data, None, 2, 3, 10, 0, out_s.ctypes.data, out_i.ctypes.data) == -27
        assert "bin_sign rows only" in err()
        assert lib.hz_index_search3(ix9._h, 0, q.ctypes.data, None, 2, 3, 2, 0, out_s.ctypes.data, out_i.ctypes.data) == -28
        # the add / read forms: the wrong one names the right one
        words, rows, first = S.binarize(v[:2]), S.prepare_rows(v[:2], "ip"), C.c_longlong(-1)
        codes, scales = S.prepare_rows_fp8(v[:2], "ip")
        assert lib.hz_index_add(h, rows.ctypes.data, 2, None, C.byref(first)) == -26 and "bin_sign" in err()
        assert lib.hz_index_add_q(h, codes.ctypes.data, scales.ctypes.data, 2, None, C.byref(first)) == -26 and "bin_sign" in err()
        assert lib.hz_index_add_br(h, words.ctypes.data, rows.ctypes.data, 2, None, C.byref(first)) == -29
        assert "hz_index_add_b" in err()
        assert lib.hz_index_add_b(ix9._h, words.ctypes.data, 2, None, C.byref(first)) == -29 and "hz_index_add_br" in err()
        assert lib.hz_index_read_state(h, None, None, None, 0) == -26 and "bin_sign" in err()
        assert ix.count == ix9.count == 64 and ix.describe()["live"] == 64  # nothing was added
    bf = str(tmp_path / "bf.hzidx")
    S.write_index(bf, v, "ip")
    with S.Index(bf, contexts=1) as plain:
        first = C.c_longlong(-1)
        assert plain._lib.hz_index_add_b(plain._h, words.ctypes.data, 2, None, C.byref(first)) == -26
        assert b"bin_sign rows, the index holds bf16" in plain._lib.hz_index_last_error()
        assert plain._lib.hz_index_read_state_b(plain._h, None, None, None, 0) == -26


# ------------------------------------------------------------------------------------------ the routes
@pytest.fixture(scope="module")
def served(tmp_path_factory):
    from transformers import BertConfig, BertModel
    from hipzap.engine import plan as PL
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path_factory.mktemp("artifacts")
    torch.manual_seed(0)
    ckpt = str(root / "enc.pth")
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), ckpt)
    emb = {"pooling": "mean", "normalize": True}
    plan = PL.export_from_checkpoint("bert-base", ckpt, batch=2, seq_len=32, embed=emb)
    rng = np.random.default_rng(38)
    c32 = rng.standard_normal((T - 3, 768)).astype(np.float32)
    q = rng.standard_normal((3, 768)).astype(np.float32)
    S.write_index(str(root / "c.hzidx"), c32, "ip", tags=(np.arange(T - 3) % 4).astype(np.uint32), dtype="bin", rescore=True)
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["live"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "plan": plan, "index": "c.hzidx", "index_writable": True, "index_reserve": 2 * T,
        "index_rescore_rows": "host"})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root / "c.hzidx"), q
    srv.close()
    app_mod.set_server(None)


def test_search_and_add_routes_equal_the_cpu_backend(served):
    client, srv, path, q = served
    new = np.random.default_rng(39).standard_normal((8, 768)).astype(np.float32)
    with S.RefIndex(path) as ref:
        def hits(**kw):
            r = client.post("/search", json=dict({"model": "live", "vectors": q.tolist(), "k": 10}, **kw))
            assert r.status_code == 200 and r.json["backend"] == "gpu" and r.json["dtype"] == "bin_sign", r.data
            return [[h["id"] for h in row] for row in r.json["results"]], r.json["refine"]
        assert hits(refine=0) == (ref.search(q, 10, refine=0)[1].tolist(), 0)
        assert hits() == (ref.search(q, 10)[1].tolist(), 128)
        assert hits(tag=2, refine=0)[0] == ref.search(q, 10, filter=(0xFFFFFFFF, 2), refine=0)[1].tolist()
        r = client.post("/index/add", json={"model": "live", "vectors": new.tolist(), "tags": [2] * 8})
        assert r.status_code == 200 and r.json["ids"] == list(range(T - 3, T + 5)), r.data  # crosses into the next tile
        ref.add(new, tags=[2] * 8)
        assert hits(tag=2, refine=0)[0] == ref.search(q, 10, filter=(0xFFFFFFFF, 2), refine=0)[1].tolist()
        assert hits(refine=40)[0] == ref.search(q, 10, refine=40)[1].tolist()
        r = client.post("/search", json={"model": "live", "vectors": new.tolist(), "k": 1})
        assert [row[0]["id"] for row in r.json["results"]] == list(range(T - 3, T + 5))
        assert client.post("/index/delete", json={"model": "live", "ids": [0]}).json["deleted"] == 1
        assert client.post("/index/save", json={"model": "live"}).json["count"] == T + 5
    index = srv.index("live", srv.text("live"))
    assert isinstance(index, S.Index) and index.dtype == "bin_sign" and index.describe()["rescore_rows"] == "host"
    assert S.file_info(path)["version"] == 9 and S.file_info(path)["live"] == T + 4
