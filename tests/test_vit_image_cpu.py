"""ViT resize plans without a GPU: `export_from_checkpoint` accepts ``resize=`` for a ViT, the plan's
first launch is the resize + patchify kernel with every later op unchanged, the default graph is what it
was, the oracle of the resize graph is the oracle of the fixed-shape graph fed the resized image, the
refused combinations, the CLI with ``--resize --embed`` and the plan-name -> checkpoint helper."""
import pytest
import torch

from hipzap import _native as N
from hipzap.engine import plan as P
from hipzap.engine.reference import run_graph_reference
from hipzap.lite import read_meta
from hipzap.models import vit
from hipzap.ops import vision as V

from test_plan_cpu import decode

RZ = (256, 224, 512, 512)


def _image(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def vit1(tmp_path_factory):
    """A 1-layer ViT-B/16 classification checkpoint on disk, its packed parameters and config."""
    torch.manual_seed(0)
    sd = vit.make_model(num_hidden_layers=1).state_dict()
    ckpt = str(tmp_path_factory.mktemp("vitimg") / "vit1.pth")
    torch.save(sd, ckpt)
    params, cfg = vit.pack_vit(sd, "cpu")
    return ckpt, params, cfg


def test_export_accepts_resize_for_vit(vit1, tmp_path):
    ckpt, _, _ = vit1
    out = P.export_from_checkpoint("vit-b16", ckpt, resize=RZ)
    assert out == ckpt + ".rz.hzplan"
    meta = read_meta(out)
    assert meta["resize"] == {"resize": 256, "crop": 224, "max_h": 512, "max_w": 512} and "embed" not in meta
    assert [i["shape"] for i in meta["inputs"]] == [[1, 786432], [1, 8]]
    assert [i["dtype"] for i in meta["inputs"]] == ["uint8", "int32"]
    from hipzap.models.bert import make_model
    torch.manual_seed(0)
    bckpt = str(tmp_path / "bert1.pth")
    torch.save(make_model(2, num_hidden_layers=1).state_dict(), bckpt)
    with pytest.raises(ValueError, match="ResNet and ViT"):
        P.export_from_checkpoint("bert-base", bckpt, resize=RZ)


def test_first_op_is_resize_patchify_and_the_rest_is_unchanged(vit1, tmp_path):
    _, params, cfg = vit1
    rz, fixed = str(tmp_path / "rz.hzplan"), str(tmp_path / "fixed.hzplan")
    m_rz = P.export_plan("vit-b16", params, dict(cfg, resize=list(RZ)), rz, batch=1)
    m_fx = P.export_plan("vit-b16", params, dict(cfg), fixed, batch=1)
    ops_rz = [(t, arg) for t, arg, _, _, _ in decode(rz)[2]]
    ops_fx = [(t, arg) for t, arg, _, _, _ in decode(fixed)[2]]
    assert m_rz["n_ops"] == m_fx["n_ops"] == len(ops_rz) == len(ops_fx)
    k_rz = [i for i, (t, _) in enumerate(ops_rz) if t == P.OP_KERNEL][0]
    k_fx = [i for i, (t, _) in enumerate(ops_fx) if t == P.OP_KERNEL][0]
    assert k_rz == k_fx
    assert ops_rz[k_rz] == (P.OP_KERNEL, N.HZ_K_RESIZE_PATCHIFY) and ops_fx[k_fx] == (P.OP_KERNEL, N.HZ_K_PREPROCESS)
    assert ops_rz[:k_rz] == ops_fx[:k_fx] and ops_rz[k_rz + 1:] == ops_fx[k_fx + 1:]
    # the parameter block of the first launch: crop 224 within 512 x 512, the ImageNet constants
    prm = V.ResizeParams.from_buffer_copy(decode(rz)[2][k_rz][3])
    assert (prm.B, prm.crop, prm.maxH, prm.maxW, prm.cap_bytes) == (1, 224, 512, 512, 786432)
    assert [round(prm.mean[c], 3) for c in range(3)] == list(V.IMAGENET_MEAN)


def test_default_graph_is_unchanged():
    g = vit.build_graph(batch=2, layers=1)
    assert len(g.inputs) == 1 and g.shape(g.inputs[0]) == (2, 3, 224, 224)
    assert g.tensors[g.inputs[0]].dtype == torch.float32 and g.tensors[g.inputs[0]].name == "input"
    assert g.nodes[0].kind == "patchify" and not any(n.kind == "resize_patchify" for n in g.nodes)
    assert g.meta == {"num_labels": 1000}
    r = vit.build_graph(batch=2, layers=1, resize=RZ)
    assert [n.kind for n in r.nodes[1:]] == [n.kind for n in g.nodes[1:]] and r.nodes[0].kind == "resize_patchify"
    assert [r.shape(t) for t in r.inputs] == [(2, 786432), (2, 8)]
    assert r.nodes[0].attrs["patch"] == 16 and r.nodes[0].attrs["mean"] == V.IMAGENET_MEAN
    assert r.meta["resize"] == {"resize": 256, "crop": 224, "max_h": 512, "max_w": 512}


def test_resize_graph_oracle_is_the_fixed_graph_on_the_resized_image(vit1):
    _, params, cfg = vit1
    img = _image(97, 131, seed=3)
    g = vit.build_graph(batch=1, **cfg, resize=RZ)
    buf, dims = V.pack_images([img], *RZ)
    got = run_graph_reference(g, params, [buf, dims])[g.outputs[0]]
    sib = vit.build_graph(batch=1, **cfg)
    x = V.resize_preprocess_reference(img)[..., :3].permute(2, 0, 1)[None].contiguous()
    want = run_graph_reference(sib, params, [x])[sib.outputs[0]]
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    # and the patch rows themselves: the oracle's layout is patchify's
    rows = V.resize_patchify_reference([img])
    assert rows.shape == (196, 768)
    assert torch.equal(rows.to(torch.bfloat16), V.patchify_reference(x))


def test_refused_combinations():
    with pytest.raises(ValueError):
        vit.build_graph(batch=1, layers=1, resize=(256, 230, 512, 512))
    with pytest.raises(ValueError):
        vit.build_graph(batch=1, layers=1, image=230, resize=(256, 230, 512, 512))
    with pytest.raises(ValueError, match="ViT-384"):
        vit.build_graph(batch=1, layers=1, image=384, resize=(384, 384, 512, 512))
    with pytest.raises(ValueError, match="the model takes 224"):
        vit.build_graph(batch=1, layers=1, resize=(256, 256, 512, 512))
    with pytest.raises(ValueError, match="conv"):
        vit.build_graph(batch=1, layers=1, patch_lowering="conv", resize=RZ)


def test_plan_cli_resize_and_embed(vit1, capsys):
    import json
    from hipzap.__main__ import main
    ckpt, _, _ = vit1
    main(["plan", "--model", "vit-b16", "--ckpt", ckpt, "--resize", "256", "--embed", "--pooling", "cls"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["out"] == ckpt + ".emb.rz.hzplan" and "resize" in line and "embed" in line
    meta = read_meta(ckpt + ".emb.rz.hzplan")
    assert meta["embed"] == {"pooling": "cls", "normalize": True, "dim": 768}
    assert meta["resize"] == {"resize": 256, "crop": 224, "max_h": 1024, "max_w": 1024}
    assert meta["output"]["shape"] == [1, 768]


def test_plan_name_maps_back_to_the_checkpoint():
    from hipzap.serve.server import plan_checkpoint
    for sfx in (".emb.rz.hzplan", ".rz.hzplan", ".emb.hzplan", ".hzplan"):
        assert plan_checkpoint("/models/x.pth" + sfx) == "/models/x.pth", sfx
