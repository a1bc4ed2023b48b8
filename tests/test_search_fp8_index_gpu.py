"""The GPU index over a version-3 (fp8) ``.hzidx`` file (csrc/index.cpp) against the host ``RefIndex``, and the
routes of a GPU server whose ``extra.index`` is such a file. Ids equal RefIndex's exactly
(tests/test_search_fp8_cpu.py asserts on the host that these scenarios are unambiguous); scores are within
``gamma(D + 1) * |scale_r| * sum_i |q_i c_ri|``; two GPU runs are compared bit for bit."""
import threading

import numpy as np
import pytest
import torch

from hipzap import search as S

import search_filter_cases as F
import search_fp8_cases as P
from search_fp8_cases import T, make

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])


def within_bound(ref, q, got):
    s, b = P.oracle_q(ref._bits, ref.scales, q)
    for qi in range(q.shape[0]):
        for j, i in enumerate(got[1][qi]):
            assert (got[0][qi, j] == -np.inf) if i < 0 else abs(float(got[0][qi, j]) - s[qi, i]) <= b[qi, i]


def test_index_on_a_version_3_file_equals_refindex(tmp_path):
    c32, q = P.big_data()
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, c32, "ip", dtype="fp8")
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        d = ix.describe()
        assert (d["dtype"], d["count"], d["capacity"], d["live"]) == ("fp8_e4m3", P.BIG_N, 4 * T, P.BIG_N)
        for Q in (1, 16, 20):  # 20 splits into 16 + 4
            for k in (1, 10):
                got, want = ix.search(q[:Q], k), ref.search(q[:Q], k)
                assert np.array_equal(got[1], want[1])
                within_bound(ref, q[:Q], got)
                assert same(ix.search(q[:Q], k), got)  # the captured program gives the eager run's bits


def test_mutations_keep_earlier_results_and_drop_programs_only_when_they_must(tmp_path):
    _, c32, q = make(T - 6, 80, 1, 33, "pos")
    tiny = make(2 * T + 15, 80, 1, 34, "pos")[1] * np.float32(1e-3)  # never near the top
    path, saved, fresh = (str(tmp_path / n) for n in ("a.hzidx", "s.hzidx", "f.hzidx"))
    S.write_index(path, c32, "ip", dtype="fp8")
    with S.Index(path, contexts=1, reserve=2 * T) as ix:
        first = ix.search(q, 10)
        assert same(ix.search(q, 10), first) and ix.describe()["programs"] == 1
        assert list(ix.add(tiny[:3])) == [T - 6, T - 5, T - 4]  # inside the last tile
        assert ix.describe()["programs"] == 1 and same(ix.search(q, 10), first)
        ix.save(saved)
        S.write_index(fresh, np.concatenate([c32, tiny[:3]]), "ip", dtype="fp8")
        assert open(saved, "rb").read() == open(fresh, "rb").read()  # add stores what write_index of the union would
        assert ix.delete([T - 5]) == 1
        ix.set_tags([T - 4], [9])
        assert ix.describe()["programs"] == 1 and same(ix.search(q, 10), first)
        ix.add(tiny[3:15])  # crosses the tile boundary
        assert ix.describe()["programs"] == 0 and ix.describe()["capacity"] == 2 * T
        assert same(ix.search(q, 10), first) and ix.describe()["programs"] == 1
        ix.add(tiny[15:])  # past the capacity: growth
        d = ix.describe()
        assert d["programs"] == 0 and d["capacity"] > 2 * T and d["count"] == 3 * T + 9
        assert same(ix.search(q, 10), first) and same(ix.search(q, 10), first)
        assert ix.search(q, 3, filter=(0xFFFFFFFF, 9))[1].tolist() == [[T - 4, -1, -1]]
        codes, tags, live, scales = ix._state()
        want = S.prepare_rows_fp8(np.concatenate([c32, tiny]), "ip")
        assert np.array_equal(codes, want[0]) and np.array_equal(u32(scales), u32(want[1]))  # growth copied both


def test_add_delete_tags_and_filters_equal_refindex(tmp_path):
    A, B, q = P.index_data()
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, A, "ip", tags=F.index_tags(F.IX_N), dtype="fp8")
    with S.Index(path, reserve=F.IX_N + 40) as ix, S.RefIndex(path) as ref:
        got, want = F.drive(ix, B, q), F.drive(ref, B, q)
        for g, w in zip(got, want):
            assert np.array_equal(g[1], w[1])
            within_bound(ref, q, g)
        d = ix.describe()
        assert (d["count"], d["live"], d["tags"], d["dtype"]) == (F.IX_N + T, F.IX_N + T - 2, True, "fp8_e4m3")
        keep, comp, rkeep, rcomp = (str(tmp_path / n) for n in ("keep.hzidx", "comp.hzidx", "rkeep.hzidx", "rcomp.hzidx"))
        ix.save(keep)
        ix.save(comp, compact=True)
        ref.save(rcomp, compact=True)
        last = ix.search(q, 10)
    for a, b in ((comp, rcomp),):
        assert np.array_equal(S.read_rows(a), S.read_rows(b)) and np.array_equal(u32(S.read_scales(a)), u32(S.read_scales(b)))
        assert np.array_equal(S.read_tags(a), S.read_tags(b)) and S.file_info(a)["version"] == 3
    with S.Index(keep) as k2:
        assert k2.describe()["live"] == F.IX_N + T - 2 and same(k2.search(q, 10), last)
    with S.Index(comp) as c2, S.RefIndex(rcomp) as r2:
        assert c2.count == F.IX_N + T - 2  # renumbered ids
        g, w = c2.search(q, 10, filter=(0xFFFFFFFF, 3)), r2.search(q, 10, filter=(0xFFFFFFFF, 3))
        assert np.array_equal(g[1], w[1])


def test_a_bf16_and_an_fp8_index_side_by_side(tmp_path):
    rng = np.random.default_rng(35)
    vec = rng.standard_normal((3 * T + 5, 768)).astype(np.float32)
    q = S.normalize_rows(rng.standard_normal((4, 768)).astype(np.float32))
    planted = [3, T - 1, 2 * T + 100, 3 * T + 4]
    vec[planted] = q * np.float32(2.5)  # a row in the query's direction (cosine: its length does not matter)
    pb, pq = str(tmp_path / "b.hzidx"), str(tmp_path / "q.hzidx")
    S.write_index(pb, vec, "cosine")
    S.write_index(pq, vec, "cosine", dtype="fp8")
    with S.Index(pb) as ib, S.Index(pq) as iq:
        sb, idb = ib.search(q, 1)
        sq, idq = iq.search(q, 1)
        assert idb[:, 0].tolist() == planted and idq[:, 0].tolist() == planted
        assert np.allclose(sb, 1.0, atol=1e-2) and np.allclose(sq, 1.0, atol=5e-2)
        assert (ib.describe()["dtype"], iq.describe()["dtype"]) == ("bf16", "fp8_e4m3")
        # 1 byte + 4 / 768 per element against 2, with the same tags, bitmap and scratch
        assert iq.describe()["device_bytes"] < 0.6 * ib.describe()["device_bytes"]
        lib = ib._lib  # each form refuses the other dtype, naming both
        one = np.zeros((1, 768), np.uint16)
        assert lib.hz_index_add(iq._h, one.ctypes.data, 1, None, None) != 0
        msg = lib.hz_index_last_error().decode()
        assert "bf16" in msg and "fp8_e4m3" in msg
        codes, scales = np.zeros((1, 768), np.uint8), np.ones(1, np.float32)
        assert lib.hz_index_add_q(ib._h, codes.ctypes.data, scales.ctypes.data, 1, None, None) != 0
        msg = lib.hz_index_last_error().decode()
        assert "bf16" in msg and "fp8_e4m3" in msg


def test_searches_are_constant_while_another_thread_mutates(tmp_path):
    _, c32, q = make(2 * T + 31, 80, 2, 36, "pos")
    extra = make(16, 80, 1, 37, "pos")[1] * np.float32(1e-3)
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, c32, "ip", dtype="fp8")
    with S.RefIndex(path) as ref:  # the mutations never reach the top 2: RefIndex answers the same at every prefix
        rid = [ref.search(q[t:t + 1], 2)[1] for t in range(2)]
    with S.Index(path) as ix:  # the adds cross a tile boundary and then outgrow the capacity of 3 tiles
        ix.delete([int(np.setdiff1d(np.arange(8), np.concatenate(rid).ravel())[0])])
        want = [ix.search(q[t:t + 1], 2) for t in range(2)]
        assert np.array_equal(want[0][1], rid[0]) and np.array_equal(want[1][1], rid[1])
        errs = []

        def searcher(t):
            try:
                for _ in range(40):
                    assert same(ix.search(q[t:t + 1], 2), want[t])
            except Exception as e:  # noqa: BLE001 - reported by the main thread
                errs.append(e)

        def mutator():
            try:
                for _ in range(20):
                    ids = ix.add(extra)
                    assert ix.delete(ids[:8]) == 8
                    ix.set_tags(ids[8:], [3] * 8)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=searcher, args=(t % 2,)) for t in range(4)] + [threading.Thread(target=mutator)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        d = ix.describe()
        assert d["count"] == 2 * T + 31 + 320 and d["live"] == d["count"] - 1 - 160 and d["capacity"] > 3 * T
        assert same(ix.search(q[:1], 2), want[0])


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
    _, c32, q = make(T - 3, 768, 3, 38, "pos")
    S.write_index(str(root / "c.hzidx"), c32, "ip", tags=(np.arange(T - 3) % 4).astype(np.uint32), dtype="fp8")
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["live"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "plan": plan, "index": "c.hzidx", "index_writable": True, "index_reserve": 2 * T})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root / "c.hzidx"), q
    srv.close()
    app_mod.set_server(None)


def test_search_with_tag_and_add_routes_equal_the_cpu_backend(served):
    client, srv, path, q = served
    new = make(8, 768, 1, 39, "pos")[1] * np.float32(0.5)
    with S.RefIndex(path) as ref:
        def hits(**kw):
            r = client.post("/search", json=dict({"model": "live", "vectors": q.tolist(), "k": 10}, **kw))
            assert r.status_code == 200 and r.json["backend"] == "gpu" and r.json["dtype"] == "fp8_e4m3", r.data
            return [[h["id"] for h in row] for row in r.json["results"]]
        assert hits() == ref.search(q, 10)[1].tolist()
        assert hits(tag=2) == ref.search(q, 10, filter=(0xFFFFFFFF, 2))[1].tolist()
        r = client.post("/index/add", json={"model": "live", "vectors": new.tolist(), "tags": [2] * 8})
        assert r.status_code == 200 and r.json["ids"] == list(range(T - 3, T + 5)), r.data  # crosses into the next tile
        ref.add(new, tags=[2] * 8)
        assert hits(tag=2) == ref.search(q, 10, filter=(0xFFFFFFFF, 2))[1].tolist()
        assert hits() == ref.search(q, 10)[1].tolist()
        for allow in (ref._live, ref._live & (ref._tags == 2)):  # host: each of these answers is forced
            assert P.index_unambiguous(ref, q, 10, allow)
    assert isinstance(srv.index("live", srv.text("live")), S.Index) and srv.index("live", srv.text("live")).dtype == "fp8_e4m3"
