"""Embedding plans without a GPU: the pooling oracle, the BERT / ViT embedding graphs, encoder-only
checkpoints, the fp32 interpreter against HF, plan export through PlanRecorder, POST /embed on the
CPU backend and the native plan server's refusal."""
import io
import os
import subprocess

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap.engine import plan as P
from hipzap.engine.reference import run_graph_reference
from hipzap.models import bert, vit
from hipzap.ops import transformer as T

from test_plan_cpu import decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERVE_PLAN = os.path.join(ROOT, "hipzap", "_lib", "hipzap-serve-plan")


# ---------------------------------------------------------------- oracle
def _st_pool(x, am, normalize=True):
    """The sentence-transformers mean pooling written out with torch ops (fp64)."""
    x, am = x.double(), am.double()
    v = (x * am[:, :, None]).sum(1) / am.sum(1, keepdim=True).clamp(min=1e-9)
    return torch.nn.functional.normalize(v, p=2, dim=1) if normalize else v


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", ["prefix", "holes", "none", "first1", "all_masked"])
def test_pool_embed_ref_is_the_sentence_transformers_formula(kind, normalize):
    B, L, D = 3, 11, 16
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, L, D, generator=g)
    am = torch.ones(B, L)
    if kind == "prefix":
        am[0, 4:], am[1, 9:] = 0, 0
    elif kind == "holes":
        am = (torch.rand(B, L, generator=g) < 0.5).float()
        am[:, 2] = 1
    elif kind == "all_masked":
        am[1] = 0
    first = int(kind == "first1")
    madd = None if kind in ("none", "first1") else (1 - am) * -1e9
    got = T.pool_embed_ref(x.reshape(B * L, D), B, L, madd, "mean", first, normalize)
    am_eff = am.clone()
    am_eff[:, :first] = 0
    want = _st_pool(x, am_eff, normalize)
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-15)
    if kind == "all_masked":
        assert (got[1] == 0).all()
    cls = T.pool_embed_ref(x.reshape(B * L, D), B, L, madd, "cls", 0, False)
    assert torch.equal(cls, x[:, 0].double())


# ---------------------------------------------------------------- graphs
def _kinds(g):
    return [(n.kind, n.attrs.get("name") or n.attrs.get("p") or n.attrs.get("w")) for n in g.nodes]


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_bert_embedding_graph(weights):
    B = 3
    g = bert.build_graph(B, weights=weights, head="embed", pooling="mean")
    assert g.nodes[-1].kind == "pool_embed" and g.shape(g.outputs[0]) == (B, 768)
    assert g.tensors[g.outputs[0]].dtype == torch.float32 and g.tensors[g.outputs[0]].external
    names = [n.attrs.get("name") for n in g.nodes]
    assert "pooler" not in names and "cls" not in names
    last_ln = [n for n in g.nodes if n.kind == "layernorm"][-1]
    assert g.nodes[-1].inputs[0] == last_ln.outputs[0] and last_ln.attrs["p"] == "l11.ln2"
    assert g.meta == {"head": "embed", "pooling": "mean", "normalize": True, "dim": 768}
    # the default graph is what it was: the same nodes with and without the head argument
    assert _kinds(bert.build_graph(B, weights=weights)) == _kinds(bert.build_graph(B, weights=weights, head="cls"))
    d = bert.build_graph(B, weights=weights)
    assert d.shape(d.outputs[0]) == (B, 4) and d.meta == {"num_labels": 2} and d.nodes[-1].attrs["name"] == "cls"
    with pytest.raises(ValueError):
        bert.build_graph(B, head="embed", pooling="max")
    with pytest.raises(ValueError):
        bert.build_graph(B, head="features")


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_vit_embedding_graph(pooling):
    B = 2
    g = vit.build_graph(B, layers=2, head="embed", pooling=pooling)
    pe, ln = g.nodes[-1], g.nodes[-2]
    assert pe.kind == "pool_embed" and ln.kind == "layernorm" and ln.attrs["p"] == "final_ln"
    assert g.shape(g.outputs[0]) == (B, 768) and not any(n.attrs.get("w") == "head" for n in g.nodes)
    if pooling == "cls":
        assert ln.attrs["rows"] == B and (pe.attrs["L"], pe.attrs["mode"]) == (1, "cls")
    else:
        assert ln.attrs["rows"] == B * 197 and (pe.attrs["L"], pe.attrs["mode"], pe.attrs["first"]) == (197, "mean", 1)
    assert _kinds(vit.build_graph(B, layers=2)) == _kinds(vit.build_graph(B, layers=2, head="cls"))
    d = vit.build_graph(B, layers=2)
    assert d.shape(d.outputs[0]) == (B, 1000) and d.meta == {"num_labels": 1000}


def test_no_resnet_matcher_sees_the_new_kind():
    from hipzap.engine import fusion
    from hipzap.engine.program import conv_pairs, qkvatt_pairs
    g = bert.build_graph(1, layers=1, head="embed")
    i = len(g.nodes) - 1
    assert fusion.plan(g, {}, fusion.default_kinds(False)) == {}
    assert i not in conv_pairs(g) and i not in conv_pairs(g).values()


# ---------------------------------------------------------------- encoder-only checkpoints
@pytest.fixture(scope="module")
def bert2():
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    m = BertModel(BertConfig(num_hidden_layers=2), add_pooling_layer=False).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "LayerNorm" in name:
                p.add_(0.3 * torch.randn_like(p))
    return m


def test_encoder_only_checkpoints_pack(bert2):
    from transformers import ViTConfig, ViTModel
    params, cfg = bert.pack_bert(bert2.state_dict(), "cpu")
    assert cfg["num_labels"] is None and cfg["layers"] == 2 and "cls" not in params and "pooler" not in params
    with pytest.raises(ValueError, match="classifier"):
        bert.build_graph(1, **dict(cfg, head="cls"))
    assert bert.build_graph(1, **dict(cfg, head="embed")).nodes[-1].kind == "pool_embed"
    vm = ViTModel(ViTConfig(num_hidden_layers=1)).eval()  # with its (unused) pooler
    vp, vc = vit.pack_vit(vm.state_dict(), "cpu")
    assert vc["num_labels"] is None and vc["layers"] == 1 and "head" not in vp
    with pytest.raises(ValueError, match="classifier"):
        vit.build_graph(1, **vc)
    assert vit.build_graph(1, **dict(vc, head="embed")).nodes[-1].kind == "pool_embed"
    # the classification layouts still pack, with their head
    cp, cc = bert.pack_bert(bert.make_model(3, num_hidden_layers=1).state_dict(), "cpu")
    assert cc["num_labels"] == 3 and "cls" in cp and "pooler" in cp


def test_interpreter_matches_hf(bert2):
    """The fp32 interpreter on the embedding graph against HF fp32 hidden states pooled by the oracle.
    The packed weights are bf16 (relative rounding 2^-9 per weight): 2e-3 absolute on unit vectors
    whose elements are ~1/sqrt(768) = 0.036 covers it; a wrong mask, pooling or layer does not."""
    params, cfg = bert.pack_bert(bert2.state_dict(), "cpu")
    B, L = 3, 40
    ids = torch.randint(0, 30000, (B, L), generator=torch.Generator().manual_seed(2))
    am = torch.ones(B, L, dtype=torch.long)
    am[1, 17:] = 0
    am[2, 1:] = 0
    inputs = bert.encode_inputs(ids, None, am)
    with torch.no_grad():
        h = bert2(input_ids=ids, attention_mask=am).last_hidden_state
    for pooling in ("mean", "cls"):
        g = bert.build_graph(B, **dict(cfg, seq_len=L, head="embed", pooling=pooling))
        out = run_graph_reference(g, params, inputs, bf16_acts=False)[g.outputs[0]]
        ref = T.pool_embed_ref(h.reshape(B * L, -1), B, L, inputs[2], pooling)
        assert out.shape == (B, 768)
        assert (out.double() - ref).abs().max() < 2e-3
        assert torch.nn.functional.cosine_similarity(out.double(), ref, dim=1).min() > 1 - 1e-4


# ---------------------------------------------------------------- plan export
def test_embedding_plan_exports_on_the_cpu(bert2, tmp_path):
    ckpt = str(tmp_path / "enc.pth")
    torch.save(bert2.state_dict(), ckpt)
    path = P.export_from_checkpoint("bert-base", ckpt, batch=2, seq_len=24, embed={"pooling": "cls", "normalize": False})
    assert path == ckpt + ".emb.hzplan" == P.plan_path(ckpt, "emb")
    hdr, meta, ops, blob = decode(path)
    assert meta["embed"] == {"pooling": "cls", "normalize": False, "dim": 768}
    assert meta["output"]["num_labels"] is None and meta["output"]["shape"] == [2, 768]
    assert meta["arch_kw"]["head"] == "embed" and meta["kind"] == "text" and meta["seq_len"] == 24
    t, kind, slot, prm, rels = ops[-1]
    assert t == P.OP_KERNEL and kind == N.HZ_K_POOL_EMBED
    pe = T.PoolEmbedParams.from_buffer_copy(prm)
    assert (pe.B, pe.L, pe.D, pe.mode, pe.normalize, pe.first) == (2, 24, 768, 0, 0, 0)
    sizes = {0: hdr["blob_len"], 1: hdr["ctx_dev"], 2: hdr["ctx_host"]}
    for _, _, _, prm, rels in ops:  # every pointer field of every op has a relocation inside its region
        for off, region, r_off in rels:
            assert 0 <= r_off < sizes[region] and off + 8 <= len(prm)
    assert {r[0] for r in rels} == {0, 8, 16}  # x, mask, out
    with pytest.raises(ValueError, match="probs"):
        P.export_from_checkpoint("bert-base", ckpt, str(tmp_path / "p.hzplan"), embed={"pooling": "mean"}, probs=True)
    params, cfg = bert.pack_bert(bert2.state_dict(), "cpu")
    with pytest.raises(ValueError, match="probs"):
        P.export_plan("bert-base", params, dict(cfg, seq_len=24, head="embed"), str(tmp_path / "q.hzplan"), probs=True)


@pytest.mark.skipif(not os.path.exists(SERVE_PLAN), reason="hipzap-serve-plan is not built")
def test_native_plan_server_refuses_an_embedding_plan(bert2, tmp_path):
    params, cfg = bert.pack_bert(bert2.state_dict(), "cpu")
    path = str(tmp_path / "e.emb.hzplan")
    P.export_plan("bert-base", params, dict(cfg, seq_len=16, head="embed"), path, batch=1)
    r = subprocess.run([SERVE_PLAN, path, "--once", path], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "is an embedding plan" in r.stderr and len(r.stderr.strip().splitlines()) == 1


# ---------------------------------------------------------------- the route (CPU backend)
@pytest.fixture(scope="module")
def client(bert2, tmp_path_factory):
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path_factory.mktemp("artifacts")
    torch.save(bert2.state_dict(), str(root / "enc.pth"))
    torch.manual_seed(0)
    torch.save(bert.make_model(2, num_hidden_layers=1).state_dict(), str(root / "cls.pth"))
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["bert-emb"] = ModelSpec(name="bert-base", key="enc.pth",
                                      extra={"embed": {"pooling": "mean", "normalize": True}, "seq_len": 32})
    st.models["bert-raw"] = ModelSpec(name="bert-base", key="enc.pth",
                                      extra={"embed": {"pooling": "cls", "normalize": False}, "seq_len": 32})
    st.models["bert-cls"] = ModelSpec(name="bert-base", key="cls.pth")
    app_mod.set_server(ModelServer(st, backend="cpu"))
    with app_mod.app.test_client() as c:
        yield c
    app_mod.set_server(None)


IDS = [[101, 2023, 2003, 1037, 3231, 102], [101, 7592, 102, 0, 0, 0]]
AM = [[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]]


def test_embed_route_json_and_npy_agree(client, bert2):
    body = {"model": "bert-emb", "input_ids": IDS, "attention_mask": AM}
    r = client.post("/embed", json=body)
    assert r.status_code == 200, r.data
    j = r.json
    assert (j["model"], j["backend"], j["batch"], j["dim"], j["pooling"], j["normalized"]) == \
        ("bert-emb", "cpu", 2, 768, "mean", True)
    e = np.asarray(j["embeddings"], np.float32)
    assert e.shape == (2, 768) and np.abs(np.linalg.norm(e.astype(np.float64), axis=1) - 1).max() < 1e-6
    rb = client.post("/embed", json=body, headers={"Accept": "application/octet-stream"})
    assert rb.status_code == 200 and rb.mimetype == "application/octet-stream"
    a = np.load(io.BytesIO(rb.data), allow_pickle=False)
    assert a.dtype == np.float32 and np.array_equal(a, e)
    with torch.no_grad():  # the transform itself: HF hidden states pooled by the oracle
        h = bert2(input_ids=torch.tensor(IDS), attention_mask=torch.tensor(AM)).last_hidden_state
    ref = T.pool_embed_ref(h.reshape(12, -1), 2, 6, (1 - torch.tensor(AM).float()) * -1e9, "mean")
    assert np.abs(a - ref.numpy()).max() < 1e-6
    raw = client.post("/embed", json={"model": "bert-raw", "input_ids": IDS, "attention_mask": AM}).json
    assert raw["pooling"] == "cls" and raw["normalized"] is False
    assert np.abs(np.asarray(raw["embeddings"]) - h[:, 0].numpy()).max() < 1e-5
    assert "POST /embed" in client.get("/").json["routes"]


def test_embed_route_refusals(client):
    r = client.post("/embed", json={"model": "bert-cls", "input_ids": IDS})
    assert r.status_code == 400 and "without extra.embed" in r.json["message"], r.data
    r = client.post("/embed", json={"model": "bert-emb", "input_ids": [list(range(1, 41))]})
    assert r.status_code == 400 and "exceeds" in r.json["message"], r.data
    r = client.post("/embed", json={"model": "bert-emb", "input_ids": [[5, 999999]]})
    assert r.status_code == 400 and "token ids" in r.json["message"], r.data
    r = client.post("/predict", json={"model": "bert-emb", "input_ids": IDS})
    assert r.status_code == 400 and "is an embedding plan: POST /embed" in r.json["message"], r.data
    r = client.post("/predict", json={"model": "bert-cls", "input_ids": IDS})
    assert r.status_code == 200 and len(r.json["probs"][0]) == 2, r.data
