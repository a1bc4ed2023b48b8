"""Live vector indexes without a GPU: the oracle's ``allow``, the version-2 ``.hzidx`` file, ``RefIndex``
add / delete / set_tags / filter / save, the mutation routes on the CPU backend and the CLI. Also asserts, on
the host, that every case of tests/test_search_filter_gpu.py is unambiguous over its passing rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hipzap import search as S

import search_filter_cases as F
from search_filter_cases import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpu_cases_are_unambiguous_over_their_passing_rows():
    for name in F.NAMES:
        bits, c32, q, k, live = F.build_case(name)
        s, b, _, _ = F.oracle(c32, q, k)
        assert F.subset_ambiguous(s, b, k, live) == 0, name
    assert {c[1] for c in F.CASES} >= {1, T - 1, T, T + 1, 3 * T + 5}
    assert {c[2] for c in F.CASES} == {8, 72, 768, 2048} and {c[3] for c in F.CASES} == {1, 3, 16}
    assert {c[4] for c in F.CASES} == {1, 10, 128}
    assert {c[6] for c in F.CASES} == {"all", "none", "last_of_partial", "mid_tile_dead", "alternating", "few_per_tile",
                                       "few_total"}
    for name, want in (("few_per_tile", lambda per, tot, k: max(per) < k < tot), ("few_total", lambda per, tot, k: tot < k)):
        _, _, _, k, live = F.build_case(name)
        per = [int(live[a:a + T].sum()) for a in range(0, live.size, T)]
        assert want(per, int(live.sum()), k), (name, per)


def test_the_index_scenario_is_unambiguous_on_the_host(tmp_path):
    """The call sequence the GPU index tests compare with ``RefIndex``: every search of it has a forced answer."""
    A, B, q = F.index_data()
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, A, "ip", tags=F.index_tags(F.IX_N))
    with S.RefIndex(path) as ix:
        F.drive(ix, B, q)
        rows, live, tags = ix._rows, ix._live, ix._tags
        s, b, _, _ = F.oracle(rows, q, 10)
        assert F.subset_ambiguous(s, b, 10, live) == 0
        assert F.subset_ambiguous(s, b, 10, live & (tags == 3)) == 0
        assert F.subset_ambiguous(s, b, 7, live & (tags & 1 == 1)) == 0 and (live & (tags == 9)).sum() == 2


def _brute(c, q, k, allow):
    out_s, out_i = np.full((q.shape[0], k), -np.inf), np.full((q.shape[0], k), -1, np.int32)
    for qi in range(q.shape[0]):
        cand = []
        for r in range(c.shape[0]):
            if allow is None or (allow[r] if allow.ndim == 1 else allow[qi, r]):
                cand.append((-(float(np.sum(c[r].astype(np.float64) * q[qi].astype(np.float64))) + 0.0), r))
        cand.sort()
        for j, (ns, r) in enumerate(cand[:k]):
            out_s[qi, j], out_i[qi, j] = -ns, r
    return out_s, out_i


def _old_search_ref(corpus, q, k):
    """search_ref as it stood before ``allow`` (copied: the bitwise yardstick of ``allow=None``)."""
    c = np.asarray(corpus, np.float64)
    q = np.asarray(q, np.float64)
    if q.ndim == 1:
        q = q[None]
    scores = np.full((q.shape[0], k), -np.inf)
    ids = np.full((q.shape[0], k), -1, np.int32)
    for i, row in enumerate(q):
        s = (c * row[None, :]).sum(axis=1) + 0.0
        order = np.argsort(-s, kind="stable")[:k]
        scores[i, :order.size] = s[order]
        ids[i, :order.size] = order
    return scores, ids


def test_search_ref_allow_against_a_brute_force_loop():
    rng = np.random.default_rng(0)
    c = S.bf16_to_f32(S.to_bf16(rng.standard_normal((60, 16)).astype(np.float32)))
    c[7] = c[3]  # a tie: the lower id first
    q = rng.standard_normal((3, 16)).astype(np.float32)
    a1 = rng.random(60) < 0.5
    a1[[3, 7]] = True
    a2 = rng.random((3, 60)) < 0.3
    a2[1] = False  # query 1: nothing allowed
    for allow in (a1, a2, np.zeros(60, bool), np.ones(60, bool)):
        for k in (1, 5, 70):
            s, i = S.search_ref(c, q, k, allow)
            bs, bi = _brute(c, q, k, allow)
            assert np.array_equal(i, bi) and i.dtype == np.int32
            assert np.allclose(s, bs, rtol=1e-12, atol=0) and np.array_equal(np.isinf(s), np.isinf(bs))
    assert (S.search_ref(c, q, 4, a2)[1][1] == -1).all()
    for k in (1, 5, 70):  # allow=None: bitwise the old function
        s, i = S.search_ref(c, q, k)
        os_, oi = _old_search_ref(c, q, k)
        assert np.array_equal(s.view(np.uint64), os_.view(np.uint64)) and np.array_equal(i, oi)
    with pytest.raises(ValueError, match="allow"):
        S.search_ref(c, q, 3, np.ones(59, bool))


def test_version_1_bytes_are_unchanged_and_version_2_round_trips(tmp_path):
    rng = np.random.default_rng(1)
    v = rng.standard_normal((70, 24)).astype(np.float32)
    labels = [f"d{i}" for i in range(70)]
    p1 = str(tmp_path / "v1.hzidx")
    hdr = S.write_index(p1, v, "cosine", labels=labels, model="m", embed={"pooling": "mean", "normalize": True, "dim": 24})
    # the version-1 file by hand: the fixed head, the JSON, zero padding, the rows
    norm = np.sqrt((v * v).sum(axis=1, dtype=np.float32), dtype=np.float32)
    rows = S.to_bf16(v / np.maximum(norm, np.float32(1e-12))[:, None])
    js = json.dumps({"dim": 24, "count": 70, "dtype": "bf16", "metric": "cosine", "model": "m",
                     "embed": {"pooling": "mean", "normalize": True, "dim": 24}, "labels": labels}).encode()
    off = -(-(S.HEAD.size + len(js)) // 4096) * 4096
    want = S.HEAD.pack(S.MAGIC, 1, len(js), off, 70, 24, 0) + js + bytes(off - S.HEAD.size - len(js)) + rows.tobytes()
    assert open(p1, "rb").read() == want and "tags_off" not in hdr
    assert S.file_info(p1) == {"version": 1, "capacity": 70, "live": 70, "tags": False}
    assert not S.read_tags(p1).any() and S.read_live(p1).all()
    # version 2
    tags = rng.integers(0, 2 ** 32, 70, dtype=np.uint64).astype(np.uint32)
    p2 = str(tmp_path / "v2.hzidx")
    hdr2 = S.write_index(p2, v, "cosine", labels=labels, model="m", tags=tags)
    got = S.read_header(p2)
    got.pop("data_off")
    assert got == hdr2 and hdr2["capacity"] == 70 and hdr2["tags_off"] % 4096 == 0 and hdr2["live_off"] % 4096 == 0
    assert S.HEAD.unpack(open(p2, "rb").read(S.HEAD.size))[1] == 2
    assert np.array_equal(S.read_rows(p2), rows) and np.array_equal(S.read_tags(p2), tags) and S.read_live(p2).all()
    assert S.file_info(p2) == {"version": 2, "capacity": 70, "live": 70, "tags": True}
    assert os.path.getsize(p2) == hdr2["live_off"] + 4 * 3
    # blocks outside the file are refused
    raw = open(p2, "rb").read()
    short = str(tmp_path / "short.hzidx")
    open(short, "wb").write(raw[:-4])
    with pytest.raises(ValueError, match="live block lies outside"):
        S.read_header(short)
    open(short, "wb").write(raw[:hdr2["tags_off"] + 8])
    with pytest.raises(ValueError, match="tags block lies outside"):
        S.read_header(short)
    for bad in ([-1] * 70, [2 ** 32] * 70, [1.5] * 70, [1] * 69):
        with pytest.raises(ValueError, match="tags"):
            S.write_index(str(tmp_path / "x.hzidx"), v, "ip", tags=np.asarray(bad))
    assert not os.path.exists(str(tmp_path / "x.hzidx"))


def test_refindex_add_delete_tags_filter_and_save(tmp_path):
    rng = np.random.default_rng(2)
    A, B = rng.standard_normal((40, 16)).astype(np.float32) * 3, rng.standard_normal((25, 16)).astype(np.float32) * 3
    q = rng.standard_normal((2, 16)).astype(np.float32)
    pa, pab = str(tmp_path / "a.hzidx"), str(tmp_path / "ab.hzidx")
    S.write_index(pa, A, "cosine")
    S.write_index(pab, np.concatenate([A, B]), "cosine")
    with S.RefIndex(pa) as ix:
        ids = ix.add(B, tags=np.arange(25))
        assert ids.dtype == np.int32 and list(ids) == list(range(40, 65)) and ix.count == 65
        assert np.array_equal(ix._bits, S.read_rows(pab))  # add(B) onto A: the bits of write_index(A u B)
        full = S.bf16_to_f32(S.read_rows(pab))
        s, i = ix.search(q, 5)
        assert np.array_equal(i, S.search_ref(full, q, 5)[1])
        best = int(i[0, 0])
        assert ix.delete([best, 41]) == 2 and ix.delete([best]) == 0 and ix.delete([]) == 0
        allow = np.ones(65, bool)
        allow[[best, 41]] = False
        s2, i2 = ix.search(q, 5)
        assert np.array_equal(i2, S.search_ref(full, q, 5, allow)[1]) and best not in i2[0]
        # filters: one pair for all queries, and one per query
        tags = np.concatenate([np.zeros(40, np.uint32), np.arange(25, dtype=np.uint32)])
        _, i3 = ix.search(q, 5, filter=(0xFFFFFFFF, 7))
        assert i3.tolist() == [[47, -1, -1, -1, -1]] * 2
        _, i4 = ix.search(q, 70, filter=[(1, 1), (0, 0)])
        assert np.array_equal(i4, S.search_ref(full, q, 70, np.stack([allow & (tags & 1 == 1), allow]))[1])
        ix.set_tags([0, 1], [7, 7])
        assert sorted(ix.search(q[:1], 5, filter=(0xFFFFFFFF, 7))[1][0].tolist()) == [-1, -1, 0, 1, 47]
        for bad in ([65], [-1], [0, 99]):
            with pytest.raises(ValueError, match=r"outside \[0, 65\)"):
                ix.delete(bad)
            with pytest.raises(ValueError, match="outside"):
                ix.set_tags(bad, [1] * len(bad))
        for bad in ((1, 2, 3), [(1, 2)] * 3, (2 ** 32, 0), (-1, 0), (1.5, 0)):
            with pytest.raises(ValueError, match="filter"):
                ix.search(q, 5, filter=bad)
        with pytest.raises(ValueError, match="no labels"):
            ix.add(B[:1], labels=["x"])
        with pytest.raises(ValueError, match=r"\[N, 16\]"):
            ix.add(np.ones((1, 24), np.float32))
        with pytest.raises(ValueError, match="non-finite"):
            ix.add(np.full((1, 16), np.nan, np.float32))
        assert ix.describe()["live"] == 63 and ix.describe()["count"] == 65
        # save: ids and tombstones kept / compacted
        keep, comp = str(tmp_path / "keep.hzidx"), str(tmp_path / "comp.hzidx")
        ix.save(keep)
        ix.save(comp, compact=True)
        want = ix.search(q, 8)
        live, tg = ix._live.copy(), ix._tags.copy()
    with S.RefIndex(keep) as k2:
        assert S.file_info(keep)["version"] == 2 and k2.count == 65 and k2.describe()["live"] == 63
        got = k2.search(q, 8)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert k2.delete([best]) == 0  # a deleted id stays dead
    with S.RefIndex(comp) as c2:
        assert c2.count == 63 and c2._live.all() and np.array_equal(c2._tags, tg[live])
        renum = np.cumsum(live) - 1
        got = c2.search(q, 8)
        assert np.array_equal(got[1], renum[want[1]]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    # labels: required iff the index has them
    pl = str(tmp_path / "l.hzidx")
    S.write_index(pl, A, "ip", labels=[f"a{i}" for i in range(40)])
    with S.RefIndex(pl) as ix:
        with pytest.raises(ValueError, match="labels are required"):
            ix.add(B[:2])
        with pytest.raises(ValueError, match="1 labels for 2 rows"):
            ix.add(B[:2], labels=["x"])
        ix.add(B[:2], labels=["x", "y"])
        ix.delete([0])
        ix.save(pl, compact=True)
    assert S.read_header(pl)["labels"][-2:] == ["x", "y"] and S.read_header(pl)["labels"][0] == "a1"
    assert S.file_info(pl)["version"] == 1  # all live, zero tags: the plain format


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "hipzap", *args], capture_output=True, text=True, cwd=ROOT, timeout=120)


def test_index_tags_option_and_info_output(tmp_path):
    v = np.random.default_rng(3).standard_normal((9, 16)).astype(np.float32)
    np.save(str(tmp_path / "v.npy"), v)
    np.save(str(tmp_path / "t.npy"), np.arange(9, dtype=np.uint32))
    out = str(tmp_path / "x.hzidx")
    r = _cli("index", "--vectors", str(tmp_path / "v.npy"), "--tags", str(tmp_path / "t.npy"), "--metric", "ip", "--out", out)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(S.read_tags(out), np.arange(9)) and np.array_equal(S.read_rows(out), S.to_bf16(v))
    r = _cli("info", out)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert (j["version"], j["capacity"], j["live"], j["tags"], j["count"]) == (2, 9, 9, True, 9)
    r = _cli("index", "--vectors", str(tmp_path / "v.npy"), "--metric", "ip", "--out", out)
    j = json.loads(_cli("info", out).stdout)
    assert (j["version"], j["capacity"], j["live"], j["tags"]) == (1, 9, 9, False)


# ---------------------------------------------------------------- the routes (CPU backend)
@pytest.fixture()
def served(tmp_path):
    from transformers import BertConfig, BertModel
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), str(root / "enc.pth"))
    rng = np.random.default_rng(5)
    corpus = rng.standard_normal((50, 768)).astype(np.float32)
    tags = (np.arange(50) % 4).astype(np.uint32)
    S.write_index(str(root / "rw.hzidx"), corpus, "cosine", labels=[f"doc{i}" for i in range(50)], tags=tags)
    S.write_index(str(root / "ro.hzidx"), corpus, "cosine")
    emb = {"pooling": "mean", "normalize": True}
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["rw"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "index": "rw.hzidx", "index_writable": True, "index_reserve": 100})
    st.models["ro"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32, "index": "ro.hzidx"})
    st.models["plain"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root), corpus, tags
    srv.close()
    app_mod.set_server(None)


def _ids(r):
    return [[h["id"] for h in row] for row in r.json["results"]]


def test_filter_and_tag_answers_equal_the_oracle_and_bad_fields_are_400(served):
    client, srv, root, corpus, tags = served
    rows = S.bf16_to_f32(S.read_rows(os.path.join(root, "rw.hzidx")))
    q = np.random.default_rng(6).standard_normal((2, 768)).astype(np.float32)
    qn = S.normalize_rows(q)
    base = {"model": "rw", "vectors": q.tolist(), "k": 6}
    r = client.post("/search", json=dict(base, tag=3))
    assert r.status_code == 200, r.data
    assert _ids(r) == S.search_ref(rows, qn, 6, tags == 3)[1].tolist()
    r = client.post("/search", json=dict(base, filter={"mask": 2, "value": 2}))
    assert _ids(r) == S.search_ref(rows, qn, 6, tags & 2 == 2)[1].tolist()
    assert _ids(client.post("/search", json=base)) == S.search_ref(rows, qn, 6)[1].tolist()
    assert _ids(client.post("/search", json=dict(base, tag=77))) == [[-1] * 6] * 2
    for body, word in ((dict(base, tag=-1), "tag"), (dict(base, tag=2 ** 32), "tag"), (dict(base, tag="3"), "tag"),
                       (dict(base, tag=1.5), "tag"), (dict(base, filter={"mask": 1}), "filter"),
                       (dict(base, filter=[1, 1]), "filter"), (dict(base, filter={"mask": -1, "value": 0}), "filter.mask"),
                       (dict(base, filter={"mask": 1, "value": 2 ** 32}), "filter.value"),
                       (dict(base, filter={"mask": 1, "value": True}), "filter.value")):
        r = client.post("/search", json=body)
        assert r.status_code == 400 and word in r.json["message"], (body.get("tag"), body.get("filter"), r.data)


def test_mutation_routes_access_rules(served):
    client, *_ = served
    v = [[0.5] * 768]
    for route, body in (("/index/add", {"vectors": v}), ("/index/delete", {"ids": [1]}), ("/index/save", {})):
        r = client.post(route, json=dict(body, model="ro"))
        assert r.status_code == 403 and "index_writable" in r.json["message"], (route, r.data)
        r = client.post(route, json=dict(body, model="plain"))
        assert r.status_code == 400 and "without extra.index" in r.json["message"], (route, r.data)
    assert client.post("/index/delete", json={"model": "rw", "ids": [50]}).status_code == 400
    assert client.post("/index/delete", json={"model": "rw", "ids": "all"}).status_code == 400
    assert client.post("/index/add", json={"model": "rw", "vectors": v}).status_code == 400  # labels are required
    assert client.post("/index/add", json={"model": "rw", "vectors": v, "labels": ["x"], "tags": [-1]}).status_code == 400
    for bad in ("x", 5, [5], {"a": 1}):
        r = client.post("/index/add", json={"model": "rw", "vectors": v, "labels": bad})
        assert r.status_code == 400 and "labels must be a list of strings" in r.json["message"], (bad, r.data)


def test_add_delete_search_then_save_and_reopen(served):
    client, srv, root, corpus, tags = served
    rng = np.random.default_rng(7)
    new = rng.standard_normal((3, 768)).astype(np.float32)
    r = client.post("/index/add", json={"model": "rw", "vectors": new.tolist(), "tags": [9, 9, 1], "labels": ["n0", "n1", "n2"]})
    assert r.status_code == 200 and r.json["ids"] == [50, 51, 52], r.data
    r = client.post("/search", json={"model": "rw", "vectors": new[:1].tolist(), "k": 2})  # the new row finds itself
    assert r.json["results"][0][0]["id"] == 50 and r.json["results"][0][0]["label"] == "n0" and r.json["count"] == 53
    r = client.post("/search", json={"model": "rw", "vectors": new[:1].tolist(), "k": 3, "tag": 9})
    assert sorted(_ids(r)[0]) == [-1, 50, 51]
    # an /embed body adds what /embed returns
    body = {"model": "rw", "input_ids": [[101, 2023, 102]], "attention_mask": [[1, 1, 1]]}
    r = client.post("/index/add", json=dict(body, labels=["text"], tags=[5]))
    assert r.status_code == 200 and r.json["ids"] == [53], r.data
    assert _ids(client.post("/search", json=dict(body, k=1)))[0] == [53]
    assert client.post("/index/delete", json={"model": "rw", "ids": [50, 53, 2]}).json == {"model": "rw", "deleted": 3}
    assert client.post("/index/delete", json={"model": "rw", "ids": [50]}).json["deleted"] == 0
    r = client.post("/search", json={"model": "rw", "vectors": new[:1].tolist(), "k": 3, "tag": 9})
    assert sorted(_ids(r)[0]) == [-1, -1, 51]
    before = client.post("/search", json={"model": "rw", "vectors": new.tolist(), "k": 10}).json["results"]
    r = client.post("/index/save", json={"model": "rw"})
    assert r.status_code == 200 and r.json["count"] == 54, r.data
    path = os.path.join(root, "rw.hzidx")
    assert S.file_info(path) == {"version": 2, "capacity": 100, "live": 51, "tags": True}
    with S.RefIndex(path) as ix:
        assert ix.labels[50:] == ["n0", "n1", "n2", "text"] and list(ix._tags[50:]) == [9, 9, 1, 5]
        s, i = ix.search(S.normalize_rows(new), 10)
        assert i.tolist() == [[h["id"] for h in row] for row in before]
