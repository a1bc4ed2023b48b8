"""The GPU index over version-6 and version-7 files (csrc/index.cpp) against the host ``RefIndex``,
and bit for bit against the GPU indexes whose scoring statements it shares: the plain fp8 index (stage one), the
plain two-stage index (both stages) and the bf16 IVF index (stage two over a candidate set that covers every passing
row). tests/test_search_ivf_fp8_cpu.py asserts on the host that every query here is forced, so ids equal the
oracle's exactly."""
import numpy as np
import pytest

from hipzap import search as S

import search_ivf_fp8_cases as V

pytestmark = pytest.mark.gpu
COVER = V.COVER_FILTER


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return V.write_files(tmp_path_factory.mktemp("ivf_fp8_gpu"))


@pytest.fixture(scope="module")
def q():
    return V.clustered_data()[1]


def test_version_6_equals_refindex_and_the_plain_fp8_index(files, q):
    with S.Index(files["v6"], contexts=1) as ix, S.RefIndex(files["v6"]) as ref, S.Index(files["p3"]) as p3, \
            S.Index(files["v5"]) as i5:
        d = ix.describe()
        assert d["dtype"] == S.FP8 and d["ivf"]["nlist"] == V.IX_LISTS and "rescore_rows" not in d and d["live"] == V.IX_N
        for n in (1, 2):
            assert np.array_equal(ix.probes(q, n), i5.probes(q, n)) and np.array_equal(ix.probes(q, n), ref.probes(q, n))
        for n in (1, 2, "all"):
            for k in (1, 10):
                assert np.array_equal(ix.search(q, k, nprobe=n)[1], ref.search(q, k, nprobe=n)[1]), (n, k)
            got = ix.search(q, 10, nprobe=n, filter=COVER)
            assert np.array_equal(got[1], ref.search(q, 10, nprobe=n, filter=COVER)[1])
        for k in (1, 10, 128):  # every list, one stage: the plain fp8 index's ids and score bits
            assert same(ix.search(q, k, nprobe="all", refine=0), p3.search(q, k))
            assert same(ix.search(q, k, nprobe="all", filter=COVER), p3.search(q, k, filter=COVER))
        assert same(ix.search(q[:1], 10, nprobe=V.IX_LISTS), p3.search(q[:1], 10))
        with pytest.raises(ValueError, match="no rescore rows"):
            ix.search(q, 10, refine=16)
        with pytest.raises(ValueError, match="IVF indexes do not take add yet"):
            ix.add(V.clustered_data()[0][:2])


@pytest.mark.parametrize("place", ["device", "host"])
def test_version_7_equals_refindex_and_the_indexes_it_shares_statements_with(files, q, tmp_path, place):
    with S.Index(files["v7"], contexts=1, rescore_rows=place) as ix, S.RefIndex(files["v7"]) as ref, \
            S.Index(files["p4"], rescore_rows=place) as p4, S.Index(files["p3"]) as p3, S.Index(files["v5"]) as i5:
        d = ix.describe()
        assert d["rescore_rows"] == place and d["dtype"] == S.FP8 and d["rescore"] == "bf16" and d["ivf"]["nprobe"] == 2
        assert np.array_equal(ix.probes(q, 2), i5.probes(q, 2))
        for n in (1, 2, "all"):
            for k in (1, 10):
                for R in (None, 40, 0):
                    got, want = ix.search(q, k, nprobe=n, refine=R), ref.search(q, k, nprobe=n, refine=R)
                    assert np.array_equal(got[1], want[1]), (n, k, R)
        for k in (1, 10, 128):
            assert same(ix.search(q, k, nprobe="all", refine=0), p3.search(q, k))          # stage one alone
            assert same(ix.search(q, k, nprobe="all", refine=128), p4.search(q, k, refine=128))  # both stages
            assert same(ix.search(q, k, nprobe="all", filter=COVER), p4.search(q, k, filter=COVER))
        # R covers every passing row of the probed lists: the bf16 IVF index's answer, ids and score bits
        for n in (1, 2):
            for k in (1, 10):
                assert same(ix.search(q, k, nprobe=n, refine=128, filter=COVER), i5.search(q, k, nprobe=n, filter=COVER)), (n, k)
        assert same(ix.search(q, 10), ix.search(q, 10, nprobe=2, refine=128))  # the defaults
        # programs: one per (Q, k, nprobe, R); mutations keep them
        progs = ix.describe()["programs"]
        first = ix.search(q, 10, nprobe=1)
        assert ix.describe()["programs"] == progs
        ix.search(q, 7, nprobe=1), ix.search(q[:3], 10, nprobe=1), ix.search(q, 10, nprobe=3), ix.search(q, 10, nprobe=1, refine=64)
        assert ix.describe()["programs"] == progs + 4
        assert same(ix.search(q, 10, nprobe=1), first) and ix.describe()["programs"] == progs + 4
        gone = [int(i) for i in first[1][:, 0]]
        assert ix.delete(gone) == ref.delete(gone) == len(set(gone)) and ix.delete(gone) == 0
        ids = [int(i) for i in first[1][:, 1]]
        ix.set_tags(ids, [77] * len(ids)), ref.set_tags(ids, [77] * len(ids))
        for n in (1, 2):
            assert np.array_equal(ix.search(q, 10, nprobe=n)[1], ref.search(q, 10, nprobe=n)[1])
            got = ix.search(q, 10, nprobe=n, filter=(0xFFFFFFFF, 77))
            assert np.array_equal(got[1], ref.search(q, 10, nprobe=n, filter=(0xFFFFFFFF, 77))[1])
        assert not np.isin(ix.search(q, 128, nprobe="all")[1], gone).any() and ix.describe()["live"] == V.IX_N - len(set(gone))
        assert ix.describe()["programs"] == progs + 4  # deletes, tags and filters are data: every program stays
        with pytest.raises(ValueError, match="IVF indexes do not take add yet"):
            ix.add(V.clustered_data()[0][:2])
        with pytest.raises(ValueError, match="compact"):
            ix.save(str(tmp_path / "c.hzidx"), compact=True)
        with pytest.raises(ValueError, match="refine must be None, 0 or an integer"):
            ix.search(q, 10, refine=5)
        out = str(tmp_path / "saved.hzidx")
        ix.save(out)
        last = [ix.search(q, 10, nprobe=n, refine=R) for n in (1, 2, "all") for R in (128, 0)]
    assert S.file_info(out)["version"] == 7 and S.file_info(out)["live"] == V.IX_N - len(set(gone))
    assert np.array_equal(S.read_rows(out), S.read_rows(files["v7"])) and np.array_equal(S.read_rescore_rows(out), S.read_rescore_rows(files["v7"]))
    assert np.array_equal(u32(S.read_scales(out)), u32(S.read_scales(files["v7"])))
    with S.Index(out, rescore_rows=place) as again:
        got = [again.search(q, 10, nprobe=n, refine=R) for n in (1, 2, "all") for R in (128, 0)]
        assert all(same(a, b) for a, b in zip(got, last))


def test_version_6_mutations_and_save(files, q, tmp_path):
    with S.Index(files["v6"], contexts=1) as ix, S.RefIndex(files["v6"]) as ref:
        first = ix.search(q, 10, nprobe=1)
        progs = ix.describe()["programs"]
        gone = [int(i) for i in first[1][:, 0]]
        assert ix.delete(gone) == ref.delete(gone)
        ids = [int(i) for i in first[1][:, 1]]
        ix.set_tags(ids, [77] * len(ids)), ref.set_tags(ids, [77] * len(ids))
        for n in (1, 2):
            assert np.array_equal(ix.search(q, 10, nprobe=n)[1], ref.search(q, 10, nprobe=n)[1])
            got = ix.search(q, 10, nprobe=n, filter=(0xFFFFFFFF, 77))
            assert np.array_equal(got[1], ref.search(q, 10, nprobe=n, filter=(0xFFFFFFFF, 77))[1])
        assert ix.describe()["programs"] == progs + 1  # (Q, 10, nprobe 2) alone is new
        out = str(tmp_path / "saved6.hzidx")
        ix.save(out)
        last = [ix.search(q, 10, nprobe=n) for n in (1, 2, "all")]
    assert S.file_info(out)["version"] == 6 and np.array_equal(S.read_rows(out), S.read_rows(files["v6"]))
    with S.Index(out) as again:
        assert all(same(again.search(q, 10, nprobe=n), w) for n, w in zip((1, 2, "all"), last))


# ------------------------------------------------------------------------------------------ the route
def test_the_search_route_takes_nprobe_and_refine_on_a_gpu_backed_model(tmp_path):
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
    S.write_index(str(tmp_path / "c5.hzidx"), v, "cosine", tags=V.index_tags(), ivf=V.IX_LISTS, nprobe=2)
    S.convert_index(str(tmp_path / "c5.hzidx"), str(tmp_path / "c7.hzidx"), "fp8", rescore=True)
    st = Settings(default_model="resnet18", artifact_root=str(tmp_path))
    st.models["ivf"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "plan": plan, "index": "c7.hzidx", "index_rescore_rows": "host"})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    try:
        with app_mod.app.test_client() as client:
            ix = None
            for n, R in ((1, 40), ("all", 0), (None, None), (2, 128)):
                body = {"model": "ivf", "vectors": q.tolist(), "k": 10, **({} if n is None else {"nprobe": n}),
                        **({} if R is None else {"refine": R})}
                r = client.post("/search", json=body)
                assert r.status_code == 200 and r.json["backend"] == "gpu" and r.json["ivf"] is True, r.data
                ix = ix or srv.index("ivf", srv.text("ivf"))
                assert isinstance(ix, S.Index) and ix.describe()["rescore_rows"] == "host"
                want = ix.search(S.normalize_rows(q), 10, nprobe=n, refine=R)  # the route normalises a cosine index's queries
                assert [[h["id"] for h in row] for row in r.json["results"]] == want[1].tolist()
                assert r.json["nprobe"] == (2 if n is None else n) and r.json["refine"] == (128 if R is None else R)
                assert r.json["dtype"] == S.FP8
                got = np.array([[h["score"] for h in row] for row in r.json["results"]], np.float32)
                assert np.array_equal(u32(got), u32(want[0]))
            assert client.post("/search", json={"model": "ivf", "vectors": q.tolist(), "refine": 5}).status_code == 400
    finally:
        srv.close()
        app_mod.set_server(None)
