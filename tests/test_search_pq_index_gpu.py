"""pq8 indexes on the GPU (csrc/index.cpp over HZ_K_SEARCH_PQLUT / HZ_K_SEARCH_PQSCAN): ``Index`` against ``RefIndex`` on
the ``inexact`` scenario (ids equal, stage-one scores within the contract's bound; tests/test_search_pq_cpu.py asserts
that no top-k there is ambiguous under it), the two-stage answers against the bf16 index bit for bit, the live
scenario with 4m's program rules, two contexts, the by-name refusals from the native side and the routes."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import search as S

import search_pq_cases as P
from search_pq_cases import T, u32

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])


def agree(ix, ref, q, k, bound, **kw):
    """ids equal the fp64 oracle's; stage-one scores within the bound of the returned rows."""
    got, want = ix.search(q, k, refine=0, **kw), ref.search(q, k, refine=0, **kw)
    assert np.array_equal(got[1], want[1]), kw
    real = got[1] >= 0
    b = np.take_along_axis(bound, np.maximum(got[1], 0).astype(np.int64), axis=1)
    # `want` is the fp64 score rounded to fp32: half an ulp more
    err = np.abs(got[0][real].astype(np.float64) - want[0][real].astype(np.float64))
    assert (err <= b[real] + np.abs(want[0][real]) * 2.0 ** -24).all(), kw
    assert (got[0][~real] == -np.inf).all()
    assert same(ix.search(q, k, refine=0, **kw), got)  # the captured program: the eager run's bits
    return got


@pytest.mark.parametrize("rescore,placement", [(False, "device"), (True, "device"), (True, "host")])
def test_live_scenario_against_refindex_with_the_program_rules(tmp_path, rescore, placement):
    A, Bv, cb, q = P.index_data()
    n = P.IX_N + T
    tags = P.index_tags(n)
    path, saved = str(tmp_path / "a.hzidx"), str(tmp_path / "s.hzidx")
    S.write_index(path, A, "ip", dtype="pq", pq_m=P.IX_M, pq_codebook=cb, rescore=rescore, tags=tags[:P.IX_N])
    with S.Index(path, contexts=2, reserve=2 * T, rescore_rows=placement) as ix, S.RefIndex(path, reserve=2 * T) as ref:
        d = ix.describe()
        assert (d["dtype"], ix.version, d["backend"], d["m"], d["dsub"], d["codebook_bytes"]) == \
            ("pq8", 11 if rescore else 10, "gpu", P.IX_M, P.IX_D // P.IX_M, 256 * P.IX_D * 4)
        assert d["scan_span"] >= 1 and (d.get("rescore_rows") == placement if rescore else "rescore_rows" not in d)
        codes = np.concatenate([S.read_rows(path), S.prepare_rows_pq(Bv, "ip", P.IX_M, cb)[0]])
        bound = P.score_oracle(codes, cb, q)[1]
        first = agree(ix, ref, q, P.IX_K, bound[:, :P.IX_N])
        assert 1 <= ix.describe()["programs"] <= 2  # one (Q, k) program in each context that has searched
        assert same(ix.search(q, P.IX_K, ctx=1, refine=0), first) and same(ix.search(q, P.IX_K, ctx=0, refine=0), first)  # two contexts
        for x in (ix, ref):  # across the tile boundary at 2T and past the capacity of 2T: growth by doubling
            assert list(x.add(Bv, tags=tags[P.IX_N:])) == list(range(P.IX_N, n))
        d = ix.describe()
        assert d["programs"] == 0 and d["capacity"] == 4 * T and d["count"] == n
        agree(ix, ref, q, P.IX_K, bound)
        agree(ix, ref, q, 40, bound)
        progs = ix.describe()["programs"]
        for x in (ix, ref):
            assert x.delete([0, 5, 5, P.IX_N + 1]) == 3
        assert ix.describe()["programs"] == progs  # deletes change device data only
        agree(ix, ref, q, P.IX_K, bound)
        agree(ix, ref, q, P.IX_K, bound, filter=(0xFFFFFFFF, 1))
        got = agree(ix, ref, q, P.IX_K, bound, filter=[(0xFFFFFFFF, 1), (0xFFFFFFFF, 77), (0, 0)])
        assert (got[1][1] == -1).all()
        for x in (ix, ref):
            x.set_tags(np.arange(10, 110), [9] * 100)
        if rescore:  # R covers every passing row (100 of them): the bf16 index's answer, bit for bit
            bf = str(tmp_path / "bf.hzidx")
            t9 = tags.copy()
            t9[10:110] = 9
            S.write_index(bf, np.concatenate([A, Bv]), "ip", tags=t9)
            with S.Index(bf, contexts=1) as plain:
                plain.delete([0, 5, P.IX_N + 1])
                want = plain.search(q, P.IX_K, filter=(0xFFFFFFFF, 9))
            assert same(ix.search(q, P.IX_K, filter=(0xFFFFFFFF, 9), refine=128), want)
            assert same(ix.search(q, P.IX_K, filter=(0xFFFFFFFF, 9)), want)  # None means 128
            assert np.array_equal(ix.search(q, P.IX_K, refine=40)[1], ref.search(q, P.IX_K, refine=40)[1])
        else:
            with pytest.raises(ValueError, match="refine must be None or 0.*pq8 index of version 10"):
                ix.search(q, P.IX_K, refine=40)
        state, rstate = ix._state(), ref._state()
        assert all(np.array_equal(a, b) for a, b in zip(state, rstate) if a is not None)
        assert np.array_equal(state[0], codes)
        ix.save(saved)
        ref.save(str(tmp_path / "r.hzidx"))
        assert open(saved, "rb").read() == open(str(tmp_path / "r.hzidx"), "rb").read()
        want = ref.search(q, P.IX_K, refine=0)
    with S.Index(saved, contexts=1, rescore_rows=placement) as again:
        assert again.version == (11 if rescore else 10) and np.array_equal(again.search(q, P.IX_K, refine=0)[1], want[1])
        compact = str(tmp_path / "c.hzidx")
        assert again.save(compact, compact=True)["count"] == n - 3
    with S.Index(compact, contexts=1) as ix, S.RefIndex(compact) as ref:
        assert np.array_equal(ix.search(q, P.IX_K, refine=0)[1], ref.search(q, P.IX_K, refine=0)[1])


def test_a_wide_index_and_batches_above_sixteen_queries(tmp_path):
    # D = 768, M = 96 and 48: the table above 64 KiB of LDS; exact arithmetic, so Index equals RefIndex bit for bit
    for M in (96, 48):
        codes, cb, q = P.make("lossless", 2 * T + 37, 768, M, 20)
        v = S.pq_decode(codes, cb)
        p = str(tmp_path / f"w{M}.hzidx")
        S.write_index(p, v, "ip", dtype="pq", pq_m=M, pq_codebook=cb, tags=(np.arange(v.shape[0]) % 7).astype(np.uint32))
        with S.Index(p, contexts=1) as ix, S.RefIndex(p) as ref:
            for Q, k in ((1, 1), (16, 128), (20, 10)):  # 20: two native calls
                for kw in ({}, {"filter": (0xFFFFFFFF, 3)}):
                    assert same(ix.search(q[:Q], k, **kw), ref.search(q[:Q], k, **kw)), (M, Q, k, kw)
            assert np.array_equal(ix.search(q, 10)[1], S.search_ref(v, q, 10)[1])  # lossless: exact search over the rows


def test_by_name_refusals_from_the_native_side(tmp_path):
    A, Bv, cb, q = P.index_data()
    v, q = A[:64], np.ascontiguousarray(q[:2])
    p10, p11 = str(tmp_path / "p10.hzidx"), str(tmp_path / "p11.hzidx")
    S.write_index(p10, v, "ip", dtype="pq", pq_m=P.IX_M, pq_codebook=cb)
    S.write_index(p11, v, "ip", dtype="pq", pq_m=P.IX_M, pq_codebook=cb, rescore=True)
    with S.Index(p10, contexts=1) as ix, S.Index(p11, contexts=1) as ix11:
        lib, h = ix._lib, ix._h
        err = lambda: lib.hz_index_last_error().decode()  # noqa: E731
        for call in (lambda: ix.neighbors([0], 3), lambda: ix.knn_graph(3), lambda: ix.cluster(2), lambda: ix.search_batch(q, 3),
                     lambda: ix.search(q, 3, nprobe=2), lambda: ix.probes(q, 2)):
            with pytest.raises(ValueError, match="a pq8 index of version 10"):
                call()
        out_s, out_i, last = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32), np.zeros(2, np.float32)
        ids = np.zeros(1, np.int32)
        assert lib.hz_index_neighbors(h, 0, ids.ctypes.data, 1, 3, 1, out_s.ctypes.data, out_i.ctypes.data) == -35
        assert "a pq8 index of version 10" in err()
        cent = np.zeros((2, P.IX_D), np.uint16)
        assert lib.hz_index_assign(h, 0, cent.ctypes.data, 2, None, out_i.ctypes.data, out_s.ctypes.data) == -38
        assert "a pq8 index of version 10" in err()
        assert lib.hz_index_search_batch(h, 0, q.ctypes.data, 2, 3, 3, out_s.ctypes.data, out_i.ctypes.data, last.ctypes.data) == -44
        assert "a pq8 index of version 10" in err()
        assert lib.hz_index_search3(h, 0, q.ctypes.data, None, 2, 3, 0, 2, out_s.ctypes.data, out_i.ctypes.data) == -34
        assert "a pq8 index of version 10" in err()
        assert lib.hz_index_probes(h, 0, q.ctypes.data, 2, 2, out_i.ctypes.data) == -34 and "pq8" in err()
        assert lib.hz_index_search3(h, 0, q.ctypes.data, None, 2, 3, 10, 0, out_s.ctypes.data, out_i.ctypes.data) == -27
        assert "pq8 rows only" in err() and "version-11" in err()
        assert lib.hz_index_search3(ix11._h, 0, q.ctypes.data, None, 2, 3, 2, 0, out_s.ctypes.data, out_i.ctypes.data) == -28
        # the add / read forms: the wrong one names the right one
        codes, rows, first = S.prepare_rows_pq(v[:2], "ip", P.IX_M, cb)[0], S.prepare_rows(v[:2], "ip"), C.c_longlong(-1)
        words = S.binarize(v[:2])
        assert lib.hz_index_add(h, rows.ctypes.data, 2, None, C.byref(first)) == -26 and "pq8" in err()
        assert lib.hz_index_add_b(h, words.ctypes.data, 2, None, C.byref(first)) == -26 and "pq8" in err()
        assert lib.hz_index_add_pr(h, codes.ctypes.data, rows.ctypes.data, 2, None, C.byref(first)) == -29
        assert "hz_index_add_p" in err()
        assert lib.hz_index_add_p(ix11._h, codes.ctypes.data, 2, None, C.byref(first)) == -29 and "hz_index_add_pr" in err()
        assert lib.hz_index_read_state(h, None, None, None, 0) == -26 and "pq8" in err()
        assert lib.hz_index_read_state_b(h, None, None, None, 0) == -26 and "pq8" in err()
        got = np.zeros_like(cb)
        assert lib.hz_index_read_codebook(h, got.ctypes.data) == 0 and np.array_equal(u32(got), u32(cb))
        assert ix.count == ix11.count == 64 and ix.describe()["live"] == 64  # nothing was added
    bf = str(tmp_path / "bf.hzidx")
    S.write_index(bf, v, "ip")
    with S.Index(bf, contexts=1) as plain:
        first = C.c_longlong(-1)
        assert plain._lib.hz_index_add_p(plain._h, codes.ctypes.data, 2, None, C.byref(first)) == -26
        assert b"pq8 rows, the index holds bf16" in plain._lib.hz_index_last_error()
        assert plain._lib.hz_index_read_state_p(plain._h, None, None, None, 0) == -26
        assert plain._lib.hz_index_read_codebook(plain._h, got.ctypes.data) == -26


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
    codes, cb, q = P.make("lossless", T - 3, 768, 48, 3)  # exact arithmetic: the GPU and the CPU backend agree bit for bit
    S.write_index(str(root / "c.hzidx"), S.pq_decode(codes, cb), "ip", tags=(np.arange(T - 3) % 4).astype(np.uint32), dtype="pq",
                  pq_m=48, pq_codebook=cb, rescore=True)
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["live"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "plan": plan, "index": "c.hzidx", "index_writable": True, "index_reserve": 2 * T,
        "index_rescore_rows": "host"})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root / "c.hzidx"), q, cb
    srv.close()
    app_mod.set_server(None)


def test_search_and_add_routes_equal_the_cpu_backend(served):
    client, srv, path, q, cb = served
    new = S.pq_decode(P.make("lossless", 8, 768, 48, 1, salt=5)[0], cb)
    with S.RefIndex(path) as ref:
        def hits(**kw):
            r = client.post("/search", json=dict({"model": "live", "vectors": q.tolist(), "k": 10}, **kw))
            assert r.status_code == 200 and r.json["backend"] == "gpu" and r.json["dtype"] == "pq8", r.data
            return [[h["id"] for h in row] for row in r.json["results"]], r.json["refine"]
        assert hits(refine=0) == (ref.search(q, 10, refine=0)[1].tolist(), 0)
        assert hits() == (ref.search(q, 10)[1].tolist(), 128)
        assert hits(tag=2, refine=0)[0] == ref.search(q, 10, filter=(0xFFFFFFFF, 2), refine=0)[1].tolist()
        for body in ({"nprobe": 2}, {"batch": True}):
            r = client.post("/search", json=dict(body, model="live", vectors=q.tolist(), k=10))
            assert r.status_code == 400 and "a pq8 index of version 11" in r.json["message"], r.data
        r = client.post("/index/add", json={"model": "live", "vectors": new.tolist(), "tags": [2] * 8})
        assert r.status_code == 200 and r.json["ids"] == list(range(T - 3, T + 5)), r.data  # crosses into the next tile
        ref.add(new, tags=[2] * 8)
        assert hits(tag=2, refine=0)[0] == ref.search(q, 10, filter=(0xFFFFFFFF, 2), refine=0)[1].tolist()
        assert hits(refine=40)[0] == ref.search(q, 10, refine=40)[1].tolist()
        assert client.post("/index/delete", json={"model": "live", "ids": [0]}).json["deleted"] == 1
        assert client.post("/index/save", json={"model": "live"}).json["count"] == T + 5
    index = srv.index("live", srv.text("live"))
    assert isinstance(index, S.Index) and index.dtype == "pq8" and index.describe()["rescore_rows"] == "host"
    assert S.file_info(path)["version"] == 11 and S.file_info(path)["live"] == T + 4
