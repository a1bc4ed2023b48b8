"""``Index.search_batch`` (csrc/index.cpp: hz_index_search_batch) and ``POST /search`` with ``"batch": true`` on the GPU
against ``Index.search``: wherever ``certain`` holds the ids are equal and the scores are bitwise equal; with the
fallback that is every query."""
import threading

import numpy as np
import pytest
import torch

from hipzap import search as S

import search_batch_cases as F
from search_batch_cases import T, make

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, rows=slice(None)):
    return np.array_equal(u32(a[0][rows]), u32(b[0][rows])) and np.array_equal(a[1][rows], b[1][rows])


@pytest.fixture()
def pair(tmp_path):
    rows, q = F.clustered()
    path = str(tmp_path / "c.hzidx")
    S.write_index(path, rows, "cosine")
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        yield ix, ref, rows, q


def test_search_batch_equals_search_wherever_it_is_certain(pair):
    ix, ref, rows, q = pair
    assert ref.search_batch(q, 10, fallback=False)[2].sum() >= 1  # the oracle certifies some query without fallback
    want = ix.search(q, 10)
    s, i, certain = ix.search_batch(q, 10, fallback=False)
    assert s.dtype == np.float32 and i.dtype == np.int32 and certain.dtype == bool and certain.sum() >= 1
    assert same((s, i), want, certain)
    s, i, certain = ix.search_batch(q, 10)
    assert certain.all() and same((s, i), want)
    for k, R in ((1, None), (10, 10), (10, 128), (128, None)):
        s, i, certain = ix.search_batch(q, k, candidates=R, fallback=False)
        assert same((s, i), ix.search(q, k), certain), (k, R)
    first = ix.search_batch(q, 10, fallback=False)
    for _ in range(20):  # the captured program of (100, 10, 42)
        again = ix.search_batch(q, 10, fallback=False)
        assert same(again, first) and np.array_equal(again[2], first[2])
    assert same(ix.search_batch(q[3], 10), (want[0][3:4], want[1][3:4]))


def test_more_ties_than_candidates_need_the_fallback(tmp_path):
    rows, q = F.duplicated()
    path = str(tmp_path / "d.hzidx")
    S.write_index(path, rows, "cosine")
    with S.Index(path) as ix:
        assert ix.search_batch(q, 10, fallback=False)[2].tolist() == [False]
        s, i, certain = ix.search_batch(q, 10)
        assert certain.tolist() == [True] and same((s, i), ix.search(q, 10)) and i[0].tolist() == list(range(10))


def test_an_ip_index(tmp_path):
    _, c32, q = make(60, 64, 5, 3, "pos")
    path = str(tmp_path / "p.hzidx")
    S.write_index(path, c32, "ip")
    with S.Index(path) as ix:
        want = ix.search(q, 10)
        assert not ix.search_batch(q, 10, fallback=False)[2].any()  # no bound on the rows: nothing is proven
        s, i, certain = ix.search_batch(q, 10, candidates=128, fallback=False)  # fewer than R rows: proven
        assert certain.all() and same((s, i), want)
        s, i, certain = ix.search_batch(q, 10)
        assert certain.all() and same((s, i), want)


def test_after_delete_and_add_across_a_tile_boundary(pair):
    ix, ref, rows, q = pair
    ix.search_batch(q, 10, ctx=0)
    programs = ix.describe()["programs"]
    gone = np.unique(ix.search(q, 10)[1][:, 0])
    assert ix.delete(gone) == ref.delete(gone)
    s, i, certain = ix.search_batch(q, 10, ctx=0)  # a delete changes device data only: the program stays
    assert ix.describe()["programs"] == programs and not np.isin(i, gone).any() and same((s, i), ix.search(q, 10))
    more = np.concatenate([q, rows[:T - F.IX_Q]])  # 1000 -> 1256 rows, past the tile boundary at 1024; each query's own vector is among them
    assert np.array_equal(ix.add(more), ref.add(more))
    s, i, certain = ix.search_batch(q, 10, fallback=False)
    assert same((s, i), ix.search(q, 10), certain) and certain.sum() >= 1 and (i >= F.IX_N).any()
    assert np.array_equal(ix.search_batch(q, 10)[1], ref.search_batch(q, 10)[1])


def test_q_above_the_per_call_maximum_is_split(pair):
    ix, ref, rows, q = pair
    whole = ix.search_batch(q, 10, fallback=False)
    assert ix._lib.hz_index_neighbors_max(ix._h, 64) == 64  # 100 queries are two calls
    try:
        split = ix.search_batch(q, 10, fallback=False)
        assert same(split, whole) and np.array_equal(split[2], whole[2])
        out_s, out_i, last = np.empty((65, 10), np.float32), np.empty((65, 10), np.int32), np.empty(65, np.float32)
        rc = ix._lib.hz_index_search_batch(ix._h, 0, q.ctypes.data, 65, 10, 42, out_s.ctypes.data, out_i.ctypes.data, last.ctypes.data)
        assert rc == -4 and b"1..64 queries a call, got 65" in ix._lib.hz_index_last_error()
    finally:
        assert ix._lib.hz_index_neighbors_max(ix._h, 1024) == 1024


def test_two_threads_on_two_contexts(pair):
    ix, ref, rows, q = pair
    want = ix.search(q, 10)
    out = {}

    def work(c):
        for _ in range(5):
            out[c] = ix.search_batch(q[c * 50:c * 50 + 50], 10, ctx=c)
    ts = [threading.Thread(target=work, args=(c,)) for c in (0, 1)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for c in (0, 1):
        assert out[c][2].all() and same(out[c], (want[0][c * 50:c * 50 + 50], want[1][c * 50:c * 50 + 50]))


def test_refused_index_kinds_and_arguments(pair, tmp_path):
    ix, ref, rows, q = pair
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must be an integer in 1..128"):
            ix.search_batch(q, k)
    with pytest.raises(ValueError, match="candidates must be"):
        ix.search_batch(q, 10, candidates=9)
    _, c32, q1 = make(300, 128, 1, 5)
    out_s, out_i, last = np.empty((1, 3), np.float32), np.empty((1, 3), np.int32), np.empty(1, np.float32)
    for name, kw, msg, code in (("q", dict(dtype="fp8"), "an fp8_e4m3 index of version 3", -44),
                                ("b", dict(dtype="bin"), "a bin_sign index of version 8", -44),
                                ("i", dict(ivf=4), "an IVF index of version 5", -44)):
        path = str(tmp_path / f"{name}.hzidx")
        S.write_index(path, c32, "ip", **kw)
        with S.Index(path) as bad:
            with pytest.raises(ValueError, match=msg):
                bad.search_batch(q1, 3)
            rc = bad._lib.hz_index_search_batch(bad._h, 0, q1.ctypes.data, 1, 3, 35, out_s.ctypes.data, out_i.ctypes.data, last.ctypes.data)
            assert rc == code and msg.encode() in bad._lib.hz_index_last_error()
    odd = str(tmp_path / "o.hzidx")
    S.write_index(odd, make(20, 72, 1, 0)[1], "ip")
    with S.Index(odd) as bad:
        q72 = np.zeros((1, 72), np.float32)
        with pytest.raises(ValueError, match="dim % 32 == 0"):
            bad.search_batch(q72, 3)
        rc = bad._lib.hz_index_search_batch(bad._h, 0, q72.ctypes.data, 1, 3, 35, out_s.ctypes.data, out_i.ctypes.data, last.ctypes.data)
        assert rc == -45 and b"dim % 32 == 0" in bad._lib.hz_index_last_error()
    rc = ix._lib.hz_index_search_batch(ix._h, 0, q.ctypes.data, 1, 3, 2, out_s.ctypes.data, out_i.ctypes.data, last.ctypes.data)
    assert rc == -28 and b"candidates must be in k..128, got 2" in ix._lib.hz_index_last_error()


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    from transformers import BertConfig, BertModel
    from hipzap.engine import plan as P
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path_factory.mktemp("artifacts")
    torch.manual_seed(0)
    ckpt = str(root / "enc.pth")
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), ckpt)
    emb = {"pooling": "mean", "normalize": True}
    plan = P.export_from_checkpoint("bert-base", ckpt, batch=2, seq_len=32, embed=emb)
    rows, q = F.clustered(n=T + 40, d=768, nq=20)
    S.write_index(str(root / "c.hzidx"), rows, "cosine", labels=[f"doc{i}" for i in range(T + 40)])
    S.write_index(str(root / "q.hzidx"), rows, "cosine", dtype="fp8")
    st = Settings(default_model="resnet18", artifact_root=str(root))
    for name in ("c", "q"):
        st.models[name] = ModelSpec(name="bert-base", key="enc.pth", batch=2,
                                    extra={"embed": emb, "seq_len": 32, "plan": plan, "index": f"{name}.hzidx"})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, q
    srv.close()
    app_mod.set_server(None)


def test_the_route_with_batch_true(served):
    client, srv, q = served
    plain = client.post("/search", json={"model": "c", "vectors": q.tolist(), "k": 5})
    r = client.post("/search", json={"model": "c", "vectors": q.tolist(), "k": 5, "batch": True})
    assert plain.status_code == r.status_code == 200 and r.json["backend"] == "gpu", r.data
    assert r.json["results"] == plain.json["results"] and r.json["certain"] == [True] * 20 and r.json["batch"] is True
    assert isinstance(srv.index("c", srv.text("c")), S.Index)
    bad = client.post("/search", json={"model": "q", "vectors": q[:1].tolist(), "batch": True})
    assert bad.status_code == 400 and "an fp8_e4m3 index of version 3" in bad.json["message"], bad.data
