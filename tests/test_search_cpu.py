"""Vector search without a GPU: the ``.hzidx`` writer and header, the oracle's order rule, the
``hipzap index`` / ``hipzap info`` commands and POST /search on the CPU backend."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hipzap import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_index_and_header_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.standard_normal((50, 24)).astype(np.float32) * 3
    path = str(tmp_path / "a.hzidx")
    labels = [f"doc {i}" for i in range(50)]
    embed = {"pooling": "mean", "normalize": True, "dim": 24}
    hdr = S.write_index(path, v, "ip", labels=labels, model="m", embed=embed)
    got = S.read_header(path)
    assert got.pop("data_off") % 4096 == 0 and got == hdr
    assert (got["dim"], got["count"], got["dtype"], got["metric"], got["model"], got["embed"], got["labels"]) == \
        (24, 50, "bf16", "ip", "m", embed, labels)
    rows = S.read_rows(path)
    assert rows.dtype == np.uint16 and rows.shape == (50, 24)
    assert np.array_equal(rows, torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))  # RNE
    assert os.path.getsize(path) == got_off(path) + 50 * 24 * 2
    assert S.read_header(path).get("labels") == labels and S.write_index(path, v, "ip")["embed"] is None
    assert "labels" not in S.read_header(path)
    with open(str(tmp_path / "bad.hzidx"), "wb") as f:
        f.write(b"not an index" * 10)
    with pytest.raises(ValueError, match="not a .hzidx"):
        S.read_header(str(tmp_path / "bad.hzidx"))


def got_off(path):
    return S.read_header(path)["data_off"]


def test_cosine_rows_have_unit_norm_within_bf16_rounding(tmp_path):
    rng = np.random.default_rng(1)
    v = (rng.standard_normal((64, 768)) * rng.uniform(1e-3, 1e3, (64, 1))).astype(np.float32)
    v[7] = 0  # max(||v||, 1e-12): a zero row stays zero
    path = str(tmp_path / "c.hzidx")
    S.write_index(path, v, "cosine")
    r = S.bf16_to_f32(S.read_rows(path)).astype(np.float64)
    norm = np.linalg.norm(r, axis=1)
    # bf16 keeps 8 significant bits: each element moves by at most 2^-8 of itself, so does the norm
    assert np.abs(np.delete(norm, 7) - 1).max() <= 2.0 ** -8 and norm[7] == 0
    unit = v[0].astype(np.float64) / np.linalg.norm(v[0].astype(np.float64))
    assert (np.abs(r[0] - unit) <= 2.0 ** -8 * np.abs(unit) + 1e-7).all()


def test_the_writer_refuses_what_the_kernels_must_not_see(tmp_path):
    p = str(tmp_path / "x.hzidx")
    v = np.ones((4, 16), np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[2, 5] = bad
        with pytest.raises(ValueError, match="row 2 has a non-finite"):
            S.write_index(p, w, "ip")
    with pytest.raises(ValueError, match="overflows bf16"):
        S.write_index(p, np.full((1, 8), 3.4e38, np.float32), "ip")
    for shape in ((4, 12), (4, 4), (4, 2056), (0, 16)):
        with pytest.raises(ValueError):
            S.write_index(p, np.ones(shape, np.float32), "ip")
    with pytest.raises(ValueError, match="metric"):
        S.write_index(p, v, "l2")
    with pytest.raises(ValueError, match="labels"):
        S.write_index(p, v, "ip", labels=["a"])
    with pytest.raises(ValueError, match="float array"):
        S.write_index(p, np.ones((4, 16), np.int32), "ip")
    assert not os.path.exists(p)


def test_search_ref_order_rule():
    c = np.zeros((6, 8), np.float32)
    c[:, 0] = [1, 3, 3, -2, 3, 0]
    q = np.zeros((1, 8), np.float32)
    q[0, 0] = 1
    s, i = S.search_ref(c, q, 4)
    assert list(i[0]) == [1, 2, 4, 0] and list(s[0]) == [3, 3, 3, 1]  # equal scores: the lower id first
    s, i = S.search_ref(c, q, 8)  # N < k: -1 / -inf past the rows
    assert list(i[0]) == [1, 2, 4, 0, 5, 3, -1, -1] and list(s[0, 6:]) == [-np.inf, -np.inf]
    # -0.0 counts as +0.0: a row scoring -0.0 does not fall behind a later row scoring +0.0
    c = np.zeros((3, 8), np.float32)
    c[0, 0], c[1, 0], c[2, 0] = -1, 1, -1
    q[0, 0] = 0.0
    s, i = S.search_ref(c, q, 3)
    assert list(i[0]) == [0, 1, 2] and not np.signbit(s).any()
    s1, i1 = S.search_ref(c, q[0], 2)  # a single query vector
    assert i1.shape == (1, 2) and i1.dtype == np.int32 and s1.dtype == np.float64


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "hipzap", *args], capture_output=True, text=True, cwd=ROOT, timeout=120)


def test_index_and_info_commands(tmp_path):
    v = np.random.default_rng(2).standard_normal((9, 16)).astype(np.float32)
    np.save(str(tmp_path / "v.npy"), v)
    json.dump([f"l{i}" for i in range(9)], open(str(tmp_path / "l.json"), "w"))
    out = str(tmp_path / "x.hzidx")
    r = _cli("index", "--vectors", str(tmp_path / "v.npy"), "--labels", str(tmp_path / "l.json"), "--metric", "ip",
             "--model", "demo", "--out", out)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert (j["out"], j["dim"], j["count"], j["metric"], j["model"], j["labels"]) == (out, 16, 9, "ip", "demo", True)
    assert np.array_equal(S.read_rows(out), S.to_bf16(v))
    r = _cli("info", out)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert (j["path"], j["dim"], j["count"], j["metric"], j["labels"][8]) == (out, 16, 9, "ip", "l8")
    r = _cli("index", "--out", out)
    assert r.returncode != 0 and "--vectors" in r.stderr


# ---------------------------------------------------------------- the route (CPU backend)
IDS = [[101, 2023, 2003, 1037, 3231, 102], [101, 7592, 102, 0, 0, 0]]
AM = [[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]]


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    from transformers import BertConfig, BertModel
    from hipzap.models import bert
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path_factory.mktemp("artifacts")
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=2), add_pooling_layer=False).eval().state_dict(),
               str(root / "enc.pth"))
    torch.save(bert.make_model(2, num_hidden_layers=1).state_dict(), str(root / "cls.pth"))
    rng = np.random.default_rng(3)
    corpus = rng.standard_normal((50, 768)).astype(np.float32)
    labels = [f"doc{i}" for i in range(50)]
    S.write_index(str(root / "c.hzidx"), corpus, "cosine", labels=labels)
    S.write_index(str(root / "ip.hzidx"), corpus, "ip")
    S.write_index(str(root / "narrow.hzidx"), corpus[:, :64], "ip")
    emb = {"pooling": "mean", "normalize": True}
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["plain"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32})
    st.models["cos"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32, "index": "c.hzidx"})
    st.models["raw-cos"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": {"pooling": "cls", "normalize": False}, "seq_len": 32, "index": str(root / "c.hzidx")})
    st.models["ip"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32, "index": "ip.hzidx"})
    st.models["narrow"] = ModelSpec(name="bert-base", key="enc.pth", batch=2,
                                    extra={"embed": emb, "seq_len": 32, "index": "narrow.hzidx"})
    st.models["cls"] = ModelSpec(name="bert-base", key="cls.pth")
    st.models["cls-ix"] = ModelSpec(name="bert-base", key="cls.pth", extra={"index": "c.hzidx"})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, str(root)
    srv.close()
    app_mod.set_server(None)


def _rows(root, name):
    return S.bf16_to_f32(S.read_rows(os.path.join(root, name)))


def test_search_route_equals_the_oracle_over_the_embed_output(served):
    client, root = served
    body = {"input_ids": IDS, "attention_mask": AM}
    emb = np.asarray(client.post("/embed", json=dict(body, model="cos")).json["embeddings"], np.float32)
    r = client.post("/search", json=dict(body, model="cos", k=5))
    assert r.status_code == 200, r.data
    j = r.json
    assert (j["model"], j["metric"], j["k"], j["count"]) == ("cos", "cosine", 5, 50) and j["timing_ms"] >= 0
    rs, ri = S.search_ref(_rows(root, "c.hzidx"), S.normalize_rows(emb), 5)
    assert [[h["id"] for h in row] for row in j["results"]] == ri.tolist()
    assert np.array_equal(np.asarray([[h["score"] for h in row] for row in j["results"]], np.float32), rs.astype(np.float32))
    assert [[h["label"] for h in row] for row in j["results"]] == [[f"doc{i}" for i in row] for row in ri]
    # the default k, an index without labels, inner product: the queries are not renormalised
    j = client.post("/search", json=dict(body, model="ip")).json
    rs, ri = S.search_ref(_rows(root, "ip.hzidx"), emb, 10)
    assert j["k"] == 10 and [[h["id"] for h in row] for row in j["results"]] == ri.tolist() and "label" not in j["results"][0][0]
    # a cosine index behind a backend that does not normalise: the route does
    raw = np.asarray(client.post("/embed", json=dict(body, model="raw-cos")).json["embeddings"], np.float32)
    assert abs(np.linalg.norm(raw[0]) - 1) > 0.1
    j = client.post("/search", json=dict(body, model="raw-cos", k=3)).json
    rs, ri = S.search_ref(_rows(root, "c.hzidx"), S.normalize_rows(raw), 3)
    assert [[h["id"] for h in row] for row in j["results"]] == ri.tolist()
    assert np.array_equal(np.asarray([[h["score"] for h in row] for row in j["results"]], np.float32), rs.astype(np.float32))
    assert "POST /search" in client.get("/").json["routes"]


def test_search_route_vectors_body_and_npy_answer(served):
    client, root = served
    rng = np.random.default_rng(4)
    q = rng.standard_normal((3, 768)).astype(np.float32)
    r = client.post("/search", json={"model": "cos", "vectors": q.tolist(), "k": 60})  # k above the 50 rows
    assert r.status_code == 200, r.data
    rs, ri = S.search_ref(_rows(root, "c.hzidx"), S.normalize_rows(q), 60)
    assert [[h["id"] for h in row] for row in r.json["results"]] == ri.tolist()
    assert r.json["results"][0][50] == {"id": -1, "score": None} and r.json["results"][0][49]["label"].startswith("doc")
    rb = client.post("/search", json={"model": "cos", "vectors": q.tolist(), "k": 4},
                     headers={"Accept": "application/octet-stream"})
    assert rb.status_code == 200 and rb.mimetype == "application/octet-stream"
    a = np.load(io.BytesIO(rb.data), allow_pickle=False)
    assert a.shape == (3, 4) and a.dtype == np.dtype([("id", "<i4"), ("score", "<f4")])
    assert np.array_equal(a["id"], ri[:, :4]) and np.array_equal(a["score"], rs[:, :4].astype(np.float32))
    one = client.post("/search", json={"model": "cos", "vectors": q[0].tolist(), "k": 2})  # a single vector
    assert one.status_code == 200 and [h["id"] for h in one.json["results"][0]] == ri[0, :2].tolist()


def test_search_route_refusals(served):
    client, _ = served
    q = [[0.5] * 768]

    def refused(body, *words, **kw):
        r = client.post("/search", json=body, **kw)
        assert r.status_code == 400, r.data
        for w in words:
            assert w in r.json["message"], r.json

    refused({"model": "plain", "input_ids": IDS}, "plain", "without extra.index")
    refused({"model": "plain", "vectors": q}, "without extra.index")
    refused({"model": "cls-ix", "vectors": q}, "without extra.embed")
    refused({"model": "cos", "vectors": [[0.5] * 64]}, "[Q, 768]", "[1, 64]")  # wrong vector width
    refused({"model": "cos", "vectors": [[0.5] * 767 + [float("nan")]]}, "non-finite")
    refused({"model": "cos", "vectors": [[0.5] * 767 + [float("inf")]]}, "non-finite")
    for k in (0, 129, -3, 2.5, "many"):
        refused({"model": "cos", "vectors": q, "k": k}, "k must be an integer in 1..128")
    refused({"model": "cos", "vectors": q}, "k must be", query_string={"k": "500"})
    refused({"model": "cos", "input_ids": IDS + IDS[:1]}, "3 inputs exceed the batch of 2")  # more than the served batch
    refused({"model": "cos", "input_ids": [list(range(1, 41))]}, "exceeds")  # /embed's own refusals still apply
    r = client.post("/search", json={"model": "narrow", "vectors": q})  # index dim != embed.dim: an error at load
    assert r.status_code == 500 and "dim 64" in r.json["message"] and "768" in r.json["message"], r.data


def test_embed_and_predict_do_not_change_with_an_index(served):
    client, _ = served
    body = {"input_ids": IDS[:1], "attention_mask": AM[:1]}
    a = client.post("/embed", json=dict(body, model="plain"), headers={"Accept": "application/octet-stream"})
    b = client.post("/embed", json=dict(body, model="cos"), headers={"Accept": "application/octet-stream"})
    assert a.status_code == b.status_code == 200 and a.data == b.data
    ja, jb = client.post("/embed", json=dict(body, model="plain")).json, client.post("/embed", json=dict(body, model="cos")).json
    for j in (ja, jb):
        j.pop("timing_ms"), j.pop("model")
    assert ja == jb
    pa = client.post("/predict", json={"model": "cls", "input_ids": IDS}).json
    pb = client.post("/predict", json={"model": "cls-ix", "input_ids": IDS}).json
    assert pa["probs"] == pb["probs"] and pa["label"] == pb["label"]
    r = client.post("/predict", json={"model": "cos", "input_ids": IDS})
    assert r.status_code == 400 and "is an embedding plan: POST /embed" in r.json["message"]
