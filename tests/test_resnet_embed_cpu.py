"""ResNet embedding plans without a GPU: the ``pool_norm`` oracle, the embedding graphs, the fp32 interpreter
against the torch module, the tail matcher on the embedding graph, plan export through PlanRecorder and its
refusals, the ``hipzap plan`` / ``hipzap index`` argument refusals and POST /embed on the CPU backend."""
import base64
import io
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hipzap import _native as N
from hipzap.__main__ import main
from hipzap.engine import fusion
from hipzap.engine import plan as P
from hipzap.engine.reference import run_graph_reference
from hipzap.models import bert, registry
from hipzap.models.resnet import build_graph, randomize_bn
from hipzap.ops import vision as V

from test_plan_cpu import decode


# ---------------------------------------------------------------- oracle
@pytest.mark.parametrize("normalize", [True, False])
def test_pool_norm_ref_is_the_mean_and_the_l2_norm(normalize):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 7, 64, generator=g)
    x[1] = 0
    got = V.pool_norm_ref(x, normalize)
    want = x.double().sum(dim=(1, 2)) / 35
    if normalize:
        want = torch.nn.functional.normalize(want, p=2, dim=1, eps=1e-12)
    assert got.dtype == torch.float64 and got.shape == (3, 64)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-15) and (got[1] == 0).all()
    # [B, C] input: the channel means themselves
    assert torch.equal(V.pool_norm_ref(want.float(), False), want.float().double())


# ---------------------------------------------------------------- graphs
def _nodes(g):
    return [(n.kind, tuple(n.inputs), tuple(n.outputs), n.slot, sorted(n.attrs.items(), key=lambda kv: kv[0]))
            for n in g.nodes]


@pytest.mark.parametrize("arch,dim", [("resnet18", 512), ("resnet50", 2048)])
@pytest.mark.parametrize("normalize", [True, False])
def test_embedding_graph(arch, dim, normalize):
    B = 3
    g = build_graph(arch, B, 1000, 224, True, head="embed", normalize=normalize)
    pn = g.nodes[-1]
    assert pn.kind == "pool_norm" and pn.attrs["normalize"] is normalize
    assert g.outputs == [pn.outputs[0]] and g.shape(g.outputs[0]) == (B, dim)
    spec = g.tensors[g.outputs[0]]
    assert spec.dtype == torch.float32 and spec.external
    assert g.shape(pn.inputs[0]) == (B, 7, 7, dim)
    assert not any(n.kind in ("pool_fc", "avgpool") or n.attrs.get("w") == "fc" for n in g.nodes)
    assert g.meta == {"head": "embed", "pooling": "mean", "normalize": normalize, "dim": dim}
    # everything before the head is the classification graph's, node for node
    c = build_graph(arch, B, 1000, 224, True)
    assert _nodes(g)[:-1] == _nodes(c)[:-1] and c.nodes[-1].kind == "pool_fc"
    assert _nodes(c) == _nodes(build_graph(arch, B, 1000, 224, True, head="cls"))
    assert c.shape(c.outputs[0]) == (B, 1, 1, 1000) and not (getattr(c, "meta", None) or {}).get("head")


def test_embedding_graph_keeps_the_resize_meta_and_refuses_other_heads():
    g = build_graph("resnet50", 1, 1000, 224, resize=(256, 224, 512, 640), head="embed")
    assert g.meta["resize"] == {"resize": 256, "crop": 224, "max_h": 512, "max_w": 640} and g.meta["dim"] == 2048
    assert [g.tensors[t].name for t in g.inputs] == ["image", "dims"] and g.nodes[-1].kind == "pool_norm"
    with pytest.raises(ValueError, match="cls"):
        build_graph("resnet50", 1, head="embed", pooling="cls")
    with pytest.raises(ValueError, match="features"):
        build_graph("resnet50", 1, head="features")
    with pytest.raises(ValueError, match="fuse_head"):
        build_graph("resnet50", 1, head="embed", fuse_head=False)
    a = registry.get("resnet50")  # the adapter passes the head (and an image size) through
    assert a.build_graph(batch=2, head="embed", image=64).nodes[-1].kind == "pool_norm"
    assert a.build_graph(batch=2).nodes[-1].kind == "pool_fc"


# ---------------------------------------------------------------- the interpreter against the torch module
def test_interpreter_matches_the_torch_module():
    """ResNet-18 at 64 px, batch 2: the fp32 interpreter (activations kept in fp32) on the embedding graph
    against ``flatten(avgpool(.))`` of the torch module, normalised by the oracle, within 1e-5.

    The packed weights are bf16, so the module carries weights that are bf16 values already and BatchNorms with
    weight 1 and variance 1 (their scale 1 / sqrt(1 + 1e-5) moves no bf16 weight: 5e-6 against a half-ulp of 2^-9),
    with random shifts and means (those fold into the fp32 bias). Packing is then lossless up to that scale, which
    the normalisation cancels to first order, and what remains is fp32 summation order: a wrong wiring, a missing
    residual or a wrong pool does not stay below 1e-5 on elements of ~1/sqrt(512) = 0.044."""
    torch.manual_seed(0)
    a = registry.get("resnet18")
    m = a.make_model().eval()
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.Conv2d, nn.Linear)):
                mod.weight.copy_(mod.weight.to(torch.bfloat16).float())
            if isinstance(mod, nn.BatchNorm2d):
                mod.bias.copy_(0.1 * torch.randn(mod.num_features, generator=gen))
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=gen))
    params, kw = a.pack(m.state_dict(), "cpu")
    x = torch.randn(2, 3, 64, 64, generator=gen)
    with torch.no_grad():
        feat = m.features(x)
        assert torch.equal(m(x), m.fc(feat))  # the classifier reads exactly these features
    g = a.build_graph(batch=2, image=64, head="embed", **kw)
    out = run_graph_reference(g, params, [x], bf16_acts=False)[g.outputs[0]]
    ref = V.pool_norm_ref(feat, True)
    err = float((out.double() - ref).abs().max())
    print(f"interpreter vs torch module: max |err| {err:.3e} on unit vectors (largest element {float(ref.abs().max()):.3f})")
    assert out.shape == (2, 512) and out.dtype == torch.float32
    assert err <= 1e-5
    raw = run_graph_reference(a.build_graph(batch=2, image=64, head="embed", normalize=False, **kw), params, [x],
                              bf16_acts=False)[g.outputs[0]]
    assert (torch.nn.functional.normalize(raw.double(), dim=1) - ref).abs().max() <= 1e-5


# ---------------------------------------------------------------- fusion
@pytest.fixture(scope="module")
def r50_cpu():
    torch.manual_seed(0)
    a = registry.get("resnet50")
    sd = randomize_bn(a.make_model()).eval().state_dict()
    params, kw = a.pack(sd, "cpu")
    return a, sd, params, kw


def test_match_tail_fires_on_the_embedding_graph_where_it_fires_on_the_classifier(r50_cpu):
    _, _, params, _ = r50_cpu
    kinds = fusion.enabled_kinds(fusion.DEFAULT)
    fired = {}
    for image in range(112, 289, 16):
        gc = build_graph("resnet50", 1, 1000, image, True)
        ge = build_graph("resnet50", 1, 1000, image, True, head="embed")
        assert len(gc.nodes) == len(ge.nodes)
        tc = [i for i in range(len(gc.nodes)) if fusion.match_tail(gc, params, i) is not None]
        te = [i for i in range(len(ge.nodes)) if fusion.match_tail(ge, params, i) is not None]
        assert tc == te, image
        pc, pe = fusion.plan(gc, params, kinds), fusion.plan(ge, params, kinds)
        assert sorted((i, f.kind, f.start, f.end) for i, f in pc.items()) == \
            sorted((i, f.kind, f.start, f.end) for i, f in pe.items()), image
        for i in te:
            f = fusion.match_tail(ge, params, i)
            assert f.kind == "tail" and f.reader == i + 1 == len(ge.nodes) - 1 and ge.nodes[f.reader].kind == "pool_norm"
        fired[image] = bool(te)
    # the last block holds (image / 32)^2 pixels: 2 .. 64 of them bind as the tail (112 -> 16, 256 -> 64, 272 -> 81)
    assert fired == {im: im <= 256 for im in range(112, 289, 16)}
    # one pixel (image 32): the channel means would not fit the block output's buffer, for either head
    for head in ("cls", "embed"):
        g = build_graph("resnet50", 1, 1000, 32, True, head=head)
        assert not any(fusion.match_tail(g, params, i) for i in range(len(g.nodes)))
    # a ResNet-18 has no bottleneck tail
    p18, _ = registry.get("resnet18").pack(registry.get("resnet18").make_model().state_dict(), "cpu")
    g18 = build_graph("resnet18", 1, 1000, 224, True, head="embed")
    assert not any(f.kind == "tail" for f in fusion.plan(g18, p18, kinds).values())


# ---------------------------------------------------------------- plan export
@pytest.fixture(scope="module")
def r18_ckpt(tmp_path_factory):
    torch.manual_seed(0)
    m = randomize_bn(registry.get("resnet18").make_model()).eval()
    root = tmp_path_factory.mktemp("r18")
    path = str(root / "r18.pth")
    torch.save(m.state_dict(), path)
    return m, root, path


def test_embedding_plan_exports_on_the_cpu(r18_ckpt):
    _, root, ckpt = r18_ckpt
    path = P.export_from_checkpoint("resnet18", ckpt, batch=2, embed={"pooling": "mean", "normalize": False})
    assert path == ckpt + ".emb.hzplan" == P.plan_path(ckpt, "emb")
    hdr, meta, ops, blob = decode(path)
    assert meta["embed"] == {"pooling": "mean", "normalize": False, "dim": 512}
    assert meta["output"]["num_labels"] is None and meta["output"]["shape"] == [2, 512] and meta["output"]["dtype"] == "float32"
    assert meta["arch_kw"]["head"] == "embed" and meta["inputs"][0]["shape"] == [2, 224, 224, 3]
    t, kind, slot, prm, rels = ops[-1]
    assert t == P.OP_KERNEL and kind == N.HZ_K_POOL_NORM == 38
    pn = V.PoolNormParams.from_buffer_copy(prm)
    assert (pn.B, pn.C, pn.HW, pn.ldo, pn.pooled, pn.normalize) == (2, 512, 49, 512, 0, 0)
    assert {r[0] for r in rels} == {0, 8} and rels[1][1] == 2  # x in the arena, out in the pinned host block
    assert N.HZ_K_POOL_FC not in [k for t, k, *_ in ops if t == P.OP_KERNEL]
    # a resize embedding plan takes the combined suffix
    rz = P.export_from_checkpoint("resnet18", ckpt, embed={"pooling": "mean"}, resize=(256, 224, 300, 400))
    assert rz == ckpt + ".emb.rz.hzplan"
    _, m2, ops2, _ = decode(rz)
    assert m2["embed"] == {"pooling": "mean", "normalize": True, "dim": 512} and m2["resize"]["max_w"] == 400
    assert [k for t, k, *_ in ops2 if t == P.OP_KERNEL][0] == N.HZ_K_RESIZE_PREPROCESS and ops2[-1][1] == 38
    assert V.PoolNormParams.from_buffer_copy(ops2[-1][3]).normalize == 1


def test_embedding_plan_refusals(r18_ckpt, tmp_path):
    _, _, ckpt = r18_ckpt
    with pytest.raises(ValueError, match="'cls'"):
        P.export_from_checkpoint("resnet18", ckpt, str(tmp_path / "c.hzplan"), embed={"pooling": "cls"})
    with pytest.raises(ValueError, match="probs"):
        P.export_from_checkpoint("resnet18", ckpt, str(tmp_path / "p.hzplan"), embed={"pooling": "mean"}, probs=True)
    assert not list(tmp_path.iterdir())


# ---------------------------------------------------------------- CLI refusals
def test_cli_refusals(r18_ckpt, tmp_path):
    _, _, ckpt = r18_ckpt
    with pytest.raises(SystemExit) as e:
        main(["plan", "--model", "resnet50", "--ckpt", str(tmp_path / "none.pth"), "--embed", "--pooling", "cls"])
    assert "--pooling cls does not apply to resnet50" in str(e.value)
    imgs, ids = str(tmp_path / "imgs.npy"), str(tmp_path / "ids.npy")
    np.save(imgs, np.zeros((2, 224, 224, 3), np.uint8))
    np.save(ids, np.zeros((2, 8), np.int64))
    out = str(tmp_path / "x.hzidx")
    plan = ckpt + ".emb.hzplan"
    if not os.path.exists(plan):
        P.export_from_checkpoint("resnet18", ckpt, embed={"pooling": "mean"})
    with pytest.raises(SystemExit) as e:
        main(["index", "--embed-plan", plan, "--images", imgs, "--ids", ids, "--out", out])
    assert "--images" in str(e.value) and "--ids" in str(e.value)
    with pytest.raises(SystemExit) as e:
        main(["index", "--vectors", imgs, "--images", imgs, "--out", out])
    assert "--images go with --embed-plan" in str(e.value)
    # a text plan takes token ids, not images
    torch.manual_seed(0)
    bp, cfg = bert.pack_bert(bert.make_model(2, num_hidden_layers=1, vocab_size=500,
                                             max_position_embeddings=64).state_dict(), "cpu")
    tplan = str(tmp_path / "t.emb.hzplan")
    P.export_plan("bert-base", bp, dict(cfg, seq_len=16, head="embed"), tplan)
    with pytest.raises(SystemExit) as e:
        main(["index", "--embed-plan", tplan, "--images", imgs, "--out", out])
    assert "is a text plan" in str(e.value)
    # a classification plan has no vectors to index
    cplan = P.export_from_checkpoint("resnet18", ckpt, str(tmp_path / "cls.hzplan"))
    with pytest.raises(SystemExit) as e:
        main(["index", "--embed-plan", cplan, "--images", imgs, "--out", out])
    assert "is not an embedding plan" in str(e.value)
    assert not os.path.exists(out)


# ---------------------------------------------------------------- the route (CPU backend)
@pytest.fixture(scope="module")
def client(r18_ckpt):
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    _, root, _ = r18_ckpt
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["r18-emb"] = ModelSpec(name="resnet18", key="r18.pth", extra={"embed": True})
    st.models["r18-raw"] = ModelSpec(name="resnet18", key="r18.pth", extra={"embed": {"normalize": False}})
    st.models["r18-cls"] = ModelSpec(name="resnet18", key="r18.pth")
    st.models["r18-bad"] = ModelSpec(name="resnet18", key="r18.pth", extra={"embed": {"pooling": "cls"}})
    app_mod.set_server(ModelServer(st, backend="cpu"))
    with app_mod.app.test_client() as c:
        yield c
    app_mod.set_server(None)


def _body(model, x):
    return {"model": model, "tensor_b64": base64.b64encode(x.numpy().tobytes()).decode(), "shape": list(x.shape)}


def test_embed_route_on_the_cpu_backend(client, r18_ckpt):
    m = r18_ckpt[0]
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    r = client.post("/embed", json=_body("r18-emb", x))
    assert r.status_code == 200, r.data
    j = r.json
    assert (j["model"], j["backend"], j["batch"], j["dim"], j["pooling"], j["normalized"]) == \
        ("r18-emb", "cpu", 3, 512, "mean", True)
    e = np.asarray(j["embeddings"], np.float32)
    assert e.shape == (3, 512) and np.abs(np.linalg.norm(e.astype(np.float64), axis=1) - 1).max() < 1e-6
    rb = client.post("/embed", json=_body("r18-emb", x), headers={"Accept": "application/octet-stream"})
    a = np.load(io.BytesIO(rb.data), allow_pickle=False)
    assert rb.status_code == 200 and a.dtype == np.float32 and np.array_equal(a, e)
    with torch.no_grad():
        feat = torch.flatten(m.avgpool(m.layer4(m.layer3(m.layer2(m.layer1(m.maxpool(m.relu(m.bn1(m.conv1(x))))))))), 1)
    assert np.abs(a - V.pool_norm_ref(feat, True).numpy()).max() < 1e-6
    raw = client.post("/embed", json=_body("r18-raw", x)).json
    assert raw["pooling"] == "mean" and raw["normalized"] is False
    assert np.abs(np.asarray(raw["embeddings"]) - feat.numpy()).max() < 1e-6 * float(feat.abs().max())
    # a uint8 image of another size goes through the host resize, as on /predict
    img = np.random.default_rng(0).integers(0, 256, (1, 97, 131, 3), dtype=np.uint8)
    r = client.post("/embed", json={"model": "r18-emb", "image_b64": base64.b64encode(img.tobytes()).decode(),
                                    "shape": list(img.shape)})
    assert r.status_code == 200 and r.json["dim"] == 512 and r.json["batch"] == 1, r.data


def test_embed_route_refusals(client):
    x = torch.zeros(1, 3, 64, 64)
    r = client.post("/embed", json=_body("r18-cls", x))
    assert r.status_code == 400 and "without extra.embed" in r.json["message"], r.data
    r = client.post("/predict", json=_body("r18-emb", x))
    assert r.status_code == 400 and "is an embedding plan: POST /embed" in r.json["message"], r.data
    r = client.post("/predict", json=_body("r18-cls", x))
    assert r.status_code == 200, r.data
    r = client.post("/embed", json=_body("r18-bad", x))
    assert r.status_code >= 400 and "pooling" in r.get_data(as_text=True)
