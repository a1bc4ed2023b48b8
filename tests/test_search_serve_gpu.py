"""POST /search on the GPU backend: a 2-layer BERT embedding plan, an index built from 64 token-id rows by
``hipzap index --embed-plan``, and each row's own token ids as the query."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hipzap import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, B = 64, 20, 4


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
    torch.save(BertModel(BertConfig(num_hidden_layers=2), add_pooling_layer=False).eval().state_dict(), ckpt)
    emb = {"pooling": "mean", "normalize": True}
    plan = P.export_from_checkpoint("bert-base", ckpt, batch=B, seq_len=32, embed=emb)
    rng = np.random.default_rng(0)
    ids = rng.integers(1000, 30000, (N, L))
    mask = np.ones((N, L), np.int64)
    mask[1::2, 14:] = 0  # every other row is a shorter sequence
    np.save(str(root / "ids.npy"), ids)
    np.save(str(root / "mask.npy"), mask)
    r = subprocess.run([sys.executable, "-m", "hipzap", "index", "--embed-plan", plan, "--ids", str(root / "ids.npy"),
                        "--mask", str(root / "mask.npy"), "--out", str(root / "c.hzidx")],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["bert-emb"] = ModelSpec(name="bert-base", key="enc.pth", batch=B,
                                      extra={"embed": emb, "seq_len": 32, "plan": plan, "index": "c.hzidx"})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, ids, mask, str(root / "c.hzidx")
    srv.close()
    app_mod.set_server(None)


@pytest.mark.gpu
def test_each_row_finds_itself_first(served):
    client, srv, ids, mask, path = served
    hdr = S.read_header(path)
    assert (hdr["count"], hdr["dim"], hdr["metric"]) == (N, 768, "cosine")
    assert hdr["embed"] == {"pooling": "mean", "normalize": True, "dim": 768} and hdr["model"] == "bert-base"
    # a row of the index is the query itself rounded to bf16 (each element moves by at most 2^-8 of itself), so
    # the fp64 score lies within 2^-8 of ||q||^2 = 1 (+- a few fp32 ulps from the normalisation: 1e-5 covers
    # them); the fp32 inner product adds at most gamma_D * sum |q_i c_i| <= gamma_D * (1 + 2^-8)
    u = 768 * 2.0 ** -24
    bound = 2.0 ** -8 + 1e-5 + u / (1 - u) * (1 + 2.0 ** -8)
    for a in range(0, N, B):
        r = client.post("/search", json={"model": "bert-emb", "input_ids": ids[a:a + B].tolist(),
                                         "attention_mask": mask[a:a + B].tolist(), "k": 3})
        assert r.status_code == 200, r.data
        j = r.json
        assert (j["metric"], j["k"], j["count"], j["backend"]) == ("cosine", 3, N, "gpu")
        for i, row in enumerate(j["results"]):
            assert row[0]["id"] == a + i, (a + i, row)
            assert abs(row[0]["score"] - 1.0) <= bound, (a + i, row[0]["score"], bound)
            assert row[0]["score"] >= row[1]["score"] >= row[2]["score"]


@pytest.mark.gpu
def test_the_route_agrees_with_the_oracle_and_stays_torch_free(served):
    from hipzap.serve.server import PlanTextBackend
    client, srv, ids, mask, path = served
    body = {"model": "bert-emb", "input_ids": ids[:B].tolist(), "attention_mask": mask[:B].tolist()}
    emb = np.asarray(client.post("/embed", json=body).json["embeddings"], np.float32)
    j = client.post("/search", json=dict(body, k=5)).json
    rows, qn = S.bf16_to_f32(S.read_rows(path)).astype(np.float64), S.normalize_rows(emb).astype(np.float64)
    rs, ri = S.search_ref(rows, qn, 5)
    got = np.asarray([[h["id"] for h in row] for row in j["results"]])
    sc = np.asarray([[h["score"] for h in row] for row in j["results"]])
    assert np.array_equal(got[:, 0], ri[:, 0])  # the self match is far from any tie
    # every returned pair against its own fp64 dot: gamma_D * sum |q_i c_i| <= gamma_D * ||q|| ||c|| <= gamma_D * 1.01
    gam = 768 * 2.0 ** -24 / (1 - 768 * 2.0 ** -24)
    for qi in range(B):
        assert len(set(got[qi])) == 5
        assert np.abs(sc[qi] - rows[got[qi]] @ qn[qi]).max() <= gam * 1.01
    r = client.post("/search", json={"model": "bert-emb", "input_ids": ids[:B + 1].tolist()})
    assert r.status_code == 400 and f"{B + 1} inputs exceed the batch of {B}" in r.json["message"]
    backend = srv.text("bert-emb")
    assert isinstance(backend, PlanTextBackend) and getattr(backend, "_torch", None) is None
    index = srv.index("bert-emb", backend)
    assert isinstance(index, S.Index) and index.describe()["programs"] >= 1
