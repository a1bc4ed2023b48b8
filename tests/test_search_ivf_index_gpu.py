"""The GPU index over an IVF file (csrc/index.cpp) against a plain GPU index of the same vectors
(bit for bit: both run the same scoring statements) and against the host ``RefIndex``. tests/test_search_ivf_cpu.py
asserts on the host that every query here is forced at nprobe 1 and 2, so the ids equal the oracle's exactly;
scores are within the suite's ``gamma`` bound."""
import numpy as np
import pytest

from hipzap import search as S

import search_ivf_cases as V
from search_ivf_cases import T

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])


def within_bound(rows32, q, got):
    s, b, _, _ = V.oracle(rows32, q, got[1].shape[1])
    for qi in range(q.shape[0]):
        for j, i in enumerate(got[1][qi]):
            assert (got[0][qi, j] == -np.inf) if i < 0 else abs(float(got[0][qi, j]) - s[qi, i]) <= b[qi, i]


@pytest.fixture()
def files(tmp_path):
    v, q = V.clustered_data()
    ivf, plain = str(tmp_path / "ivf.hzidx"), str(tmp_path / "plain.hzidx")
    S.write_index(plain, v, "cosine", tags=V.index_tags())
    S.write_index(ivf, v, "cosine", tags=V.index_tags(), ivf=V.IX_LISTS, nprobe=2, ivf_seed=1)
    return v, q, ivf, plain


def test_probes_equal_a_plain_index_over_the_centroids(files, tmp_path):
    v, q, path, plain = files
    cent = str(tmp_path / "cent.hzidx")
    S.write_index(cent, S.bf16_to_f32(S.read_ivf(path)["centroids"]), "ip")  # bf16 values: stored as they are
    assert np.array_equal(S.read_rows(cent), S.read_ivf(path)["centroids"])
    with S.Index(path) as ix, S.Index(cent) as cx, S.RefIndex(path) as ref:
        for n in (1, 2, V.IX_LISTS):
            got = ix.probes(q, n)
            assert got.dtype == np.int32 and np.array_equal(got, cx.search(q, n)[1])
        assert np.array_equal(ix.probes(q, 2), ref.probes(q, 2))  # forced on the host (test_search_ivf_cpu.py)
        assert np.array_equal(ix.probes(q, 2), ix.probes(q, 2))


def test_every_list_equals_the_plain_index_bit_for_bit(files):
    v, q, path, plain = files
    with S.Index(path) as ix, S.Index(plain) as px:
        d = ix.describe()
        assert d["count"] == V.IX_N and d["live"] == V.IX_N and d["capacity"] % T == 0 and d["capacity"] >= 3 * T
        assert d["ivf"]["nlist"] == V.IX_LISTS and d["ivf"]["nprobe"] == 2 and d["ivf"]["tiles"] == d["capacity"] // T
        for k in (1, 10, 128):
            assert same(ix.search(q, k, nprobe="all"), px.search(q, k))
            assert same(ix.search(q, k, nprobe="all", filter=(0xFFFFFFFF, 3)), px.search(q, k, filter=(0xFFFFFFFF, 3)))
        assert same(ix.search(q, 10, nprobe=V.IX_LISTS), px.search(q, 10))
        assert same(ix.search(q[:1], 10, nprobe="all"), px.search(q[:1], 10))
        gone = [int(px.search(q, 1)[1][0, 0]), 5]
        assert ix.delete(gone) == px.delete(gone) == 2 and ix.delete(gone) == 0
        for k in (1, 10, 128):
            assert same(ix.search(q, k, nprobe="all"), px.search(q, k))
        assert ix.describe()["live"] == V.IX_N - 2
        with pytest.raises(ValueError, match="outside"):
            ix.delete([V.IX_N])


def test_nprobe_answers_equal_refindex(files, tmp_path):
    v, q, path, plain = files
    with S.Index(path, contexts=1) as ix, S.RefIndex(path) as ref:
        for n in (1, 2):
            for k in (1, 10):
                got, want = ix.search(q, k, nprobe=n), ref.search(q, k, nprobe=n)
                assert np.array_equal(got[1], want[1]), (n, k)
                within_bound(ref._rows, q, got)
            got = ix.search(q, 10, nprobe=n, filter=(0xFFFFFFFF, 3))
            assert np.array_equal(got[1], ref.search(q, 10, nprobe=n, filter=(0xFFFFFFFF, 3))[1])
        assert same(ix.search(q, 10), ix.search(q, 10, nprobe=2))  # None: the header's default
        # a second (Q, k, nprobe) builds its own program and the first still replays
        progs = ix.describe()["programs"]
        first = ix.search(q, 10, nprobe=1)
        ix.search(q, 7, nprobe=1), ix.search(q[:3], 10, nprobe=1), ix.search(q, 10, nprobe=3)
        assert ix.describe()["programs"] == progs + 3
        assert same(ix.search(q, 10, nprobe=1), first) and ix.describe()["programs"] == progs + 3
        # set_tags, then a filtered search; the captured programs stay
        ids = [int(i) for i in first[1][:, 0]]
        ix.set_tags(ids, [77] * len(ids)), ref.set_tags(ids, [77] * len(ids))
        got, want = ix.search(q, 10, nprobe=1, filter=(0xFFFFFFFF, 77)), ref.search(q, 10, nprobe=1, filter=(0xFFFFFFFF, 77))
        assert np.array_equal(got[1], want[1]) and (got[1][:, 0] == ids).all() and ix.describe()["programs"] == progs + 3
        # what an IVF index does not take
        with pytest.raises(ValueError, match="IVF indexes do not take add yet"):
            ix.add(v[:2])
        with pytest.raises(ValueError, match="compact"):
            ix.save(str(tmp_path / "c.hzidx"), compact=True)
        with pytest.raises(ValueError, match="no rescore rows"):
            ix.search(q, 10, refine=16)
        with pytest.raises(ValueError, match="nprobe must be an integer"):
            ix.search(q, 10, nprobe=0)
        # save and reopen: the same answers, the tags and a delete kept
        assert ix.delete(ids[:1]) == ref.delete(ids[:1]) == 1
        out = str(tmp_path / "saved.hzidx")
        ix.save(out)
        last = [ix.search(q, 10, nprobe=n) for n in (1, 2, "all")]
    assert S.file_info(out)["version"] == 5 and S.file_info(out)["live"] == V.IX_N - 1
    with S.Index(out) as again:
        for n, want in zip((1, 2, "all"), last):
            assert same(again.search(q, 10, nprobe=n), want)
    with S.Index(plain) as px:
        with pytest.raises(ValueError, match="needs an IVF index"):
            px.search(q, 10, nprobe=1)


# ------------------------------------------------------------------------------------------ the route
def test_the_search_route_takes_nprobe_on_a_gpu_backed_model(files, tmp_path):
    import torch
    from transformers import BertConfig, BertModel
    from hipzap.engine import plan as P
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    torch.manual_seed(0)
    ckpt = str(tmp_path / "enc.pth")
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), ckpt)
    emb = {"pooling": "mean", "normalize": True}
    plan = P.export_from_checkpoint("bert-base", ckpt, batch=2, seq_len=32, embed=emb)
    v, q = V.clustered_data(d=768)
    S.write_index(str(tmp_path / "c.hzidx"), v, "cosine", tags=V.index_tags(), ivf=V.IX_LISTS, nprobe=2, ivf_seed=1)
    st = Settings(default_model="resnet18", artifact_root=str(tmp_path))
    st.models["ivf"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "plan": plan, "index": "c.hzidx", "index_writable": True})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    try:
        with app_mod.app.test_client() as client:
            ix = None
            for n in (1, "all", None):
                body = {"model": "ivf", "vectors": q.tolist(), "k": 10, **({} if n is None else {"nprobe": n})}
                r = client.post("/search", json=body)
                assert r.status_code == 200 and r.json["backend"] == "gpu" and r.json["ivf"] is True, r.data
                ix = ix or srv.index("ivf", srv.text("ivf"))
                assert isinstance(ix, S.Index)
                want = ix.search(S.normalize_rows(q), 10, nprobe=n)  # the route normalises a cosine index's queries
                assert [[h["id"] for h in row] for row in r.json["results"]] == want[1].tolist()
                assert r.json["nprobe"] == (2 if n is None else n)
                got = np.array([[h["score"] for h in row] for row in r.json["results"]], np.float32)
                assert np.array_equal(u32(got), u32(want[0]))
            r = client.post("/index/add", json={"model": "ivf", "vectors": q[:1].tolist()})
            assert r.status_code == 400 and "IVF indexes do not take add yet" in r.json["message"]
            assert client.post("/search", json={"model": "ivf", "vectors": q.tolist(), "nprobe": 0}).status_code == 400
    finally:
        srv.close()
        app_mod.set_server(None)
