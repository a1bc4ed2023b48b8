"""The ResNet embedding head on the GPU: ``pool_norm_kernel`` (csrc/vision.hip, kind 38) against the fp64
oracle, its pad columns, its independence of the batch around an image and the launcher's refusals; the
ResNet-18 / ResNet-50 embedding engines against the fp32 torch module; the bs=1 program next to the
classifier's; ``.emb.hzplan`` / ``.emb.rz.hzplan`` plans against the torch-built engine, bit for bit; and
``POST /embed``, ``/index/add`` and ``/search`` with image bodies."""
import base64
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.engine import fusion
from hipzap.engine import plan as P
from hipzap.engine.engine import Engine
from hipzap.engine.program import ExecContext
from hipzap.models import registry
from hipzap.models.resnet import build_graph, randomize_bn
from hipzap.ops import vision as V
from hipzap.ops.conv import to_blocked

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet50_bs1_graph.json")


# ---------------------------------------------------------------- the kernel against the fp64 oracle
def _bound(x):
    """x logical [B, H, W, C] (or [B, C] channel means): per element HW * 2^-23 * mean over the pixels of |x| +
    2^-24 * |ref| (the fp32 recursive-sum bound for any order, the multiplication by 1 / HW and the final
    rounding -- tests/test_embed_gpu.py derives it the same way), and the un-normalised fp64 reference."""
    ref = V.pool_norm_ref(x, False)
    hw = x.shape[1] * x.shape[2] if x.dim() == 4 else 1
    return hw * 2.0 ** -23 * V.pool_norm_ref(x.float().abs(), False) + 2.0 ** -24 * ref.abs(), ref


def _check(out, x, normalize):
    out = out.double().cpu()
    bound, ref = _bound(x)
    C_ = ref.shape[1]
    assert out.shape == ref.shape and torch.isfinite(out).all()
    if not normalize:
        err = (out - ref).abs()
        print(f"max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert (err <= bound).all()
        return
    nrm = ref.norm(dim=1, keepdim=True)
    live = nrm[:, 0] > 0
    err = (out - ref / nrm.clamp(min=1e-12)).abs()[live]
    lim = (3 * bound / nrm.clamp(min=1e-12))[live]
    print(f"normalised: max err/limit {float((err / lim.clamp(min=1e-300)).max()):.3f}, "
          f"max | ||out|| - 1 | {float((out[live].norm(dim=1) - 1).abs().max()):.3e}")
    assert ((out[live].norm(dim=1) - 1).abs() <= C_ * 2.0 ** -23).all()
    assert (err <= lim).all()
    assert (out[~live] == 0).all()


BLOCKED = [(1, 1, 32), (5, 4, 64), (2, 9, 96), (3, 49, 512), (1, 49, 2048), (2, 64, 2048), (2, 100, 2048)]
POOLED = [(1, 512), (2, 2048)]


def _images(B, HW, Cc):
    """randn + 0.25 rounded to bf16, logical [B, HW, 1, C]; image 0 of a batch is all zero."""
    g = torch.Generator().manual_seed(B * 1000 + HW * 7 + Cc)
    x = (torch.randn(B, HW, 1, Cc, generator=g) + 0.25).to(torch.bfloat16)
    if B > 1:
        x[0] = 0
    return x


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B,HW,Cc", BLOCKED)
def test_kernel_blocked_matches_the_fp64_oracle(B, HW, Cc, normalize):
    x = _images(B, HW, Cc)
    out = V.pool_norm(x.to(DEV), normalize)
    torch.cuda.synchronize()
    assert out.shape == (B, Cc) and out.dtype == torch.float32
    _check(out, x, normalize)
    if B > 1:
        assert (out[0].cpu().view(torch.int32) == 0).all()  # an all-zero image: exactly zero, normalised or not
    # the already blocked input is the same launch
    again = V.pool_norm(to_blocked(x.to(DEV)), normalize, blocked_input=True)
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B,Cc", POOLED)
def test_kernel_pooled_matches_the_fp64_oracle(B, Cc, normalize):
    g = torch.Generator().manual_seed(B + Cc)
    x = (torch.randn(B, Cc, generator=g) + 0.25).to(torch.bfloat16).float()
    if B > 1:
        x[0] = 0
    out = V.pool_norm(x.to(DEV), normalize)
    torch.cuda.synchronize()
    _check(out, x, normalize)
    if not normalize:  # the channel means themselves, bit for bit
        assert torch.equal(out.cpu().view(torch.int32), x.view(torch.int32))
    if B > 1:
        assert (out[0].cpu().view(torch.int32) == 0).all()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("pad", [4, 3])  # rows 16-B aligned (vector stores) and not (scalar stores)
def test_kernel_leaves_the_pad_columns(pad, normalize):
    B, HW, Cc = 3, 9, 96
    x = _images(B, HW, Cc)
    buf = torch.full((B, Cc + pad), 7.0, device=DEV)
    out = V.pool_norm(x.to(DEV), normalize, out=buf)
    torch.cuda.synchronize()
    assert (buf[:, Cc:] == 7.0).all()
    _check(out, x, normalize)
    tight = V.pool_norm(x.to(DEV), normalize)
    torch.cuda.synchronize()
    assert torch.equal(out.contiguous().view(torch.int32), tight.view(torch.int32))


@pytest.mark.parametrize("Cc", [512, 2048])
def test_an_image_does_not_depend_on_its_batch(Cc):
    HW = 49
    g = torch.Generator().manual_seed(9 + Cc)
    img = (torch.randn(1, HW, 1, Cc, generator=g) + 0.25).to(torch.bfloat16)
    x5 = (torch.randn(5, HW, 1, Cc, generator=g) + 0.25).to(torch.bfloat16)
    x5[3] = img[0]
    for normalize in (False, True):
        a = V.pool_norm(img.to(DEV), normalize)
        b = V.pool_norm(x5.to(DEV), normalize)
        b2 = V.pool_norm(x5.to(DEV), normalize)
        torch.cuda.synchronize()
        assert torch.equal(a[0].view(torch.int32), b[3].view(torch.int32))
        assert torch.equal(b.view(torch.int32), b2.view(torch.int32))
        # the pooled form of the same means: the same normalisation, bit for bit
        means = V.pool_norm(x5.to(DEV), False)
        p = V.pool_norm(means, normalize)
        torch.cuda.synchronize()
        assert torch.equal(p.view(torch.int32), b.view(torch.int32))


REFUSALS = ["x=null", "out=null", "x+2", "out+4", "B=0", "HW=0", "C=16", "C=48", "C=2080", "ldo<C"]


@pytest.mark.parametrize("what", REFUSALS)
def test_launcher_refuses_and_touches_nothing(what):
    B, HW, Cc = 2, 4, 64
    x = torch.full((B * HW * 2080 + 16,), 1.0, dtype=torch.bfloat16, device=DEV)
    out = torch.full((B, 2080 + 8), 7.0, device=DEV)
    prm = V.PoolNormParams(x.data_ptr(), out.data_ptr(), B, Cc, HW, out.stride(0), 0, 1)
    if what == "x=null":
        prm.x = None
    elif what == "out=null":
        prm.out = None
    elif what == "x+2":
        prm.x = x.data_ptr() + 2
    elif what == "out+4":
        prm.out = out.data_ptr() + 4
    elif what == "B=0":
        prm.B = 0
    elif what == "HW=0":
        prm.HW = 0
    elif what == "ldo<C":
        prm.ldo = Cc - 4
    else:
        prm.C = int(what[2:])
    rc = N.lib().hz_launch_kernel(N.HZ_K_POOL_NORM, C.byref(prm), N.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert (out == 7.0).all() and (x == 1.0).all()


# ---------------------------------------------------------------- engines against the fp32 torch module
def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1)


def _model(arch):
    torch.manual_seed(0)
    return randomize_bn(registry.get(arch).make_model()).eval()


@pytest.fixture(scope="module")
def nets():
    """Per (arch, image): the module's state_dict, a batch of 4 fp32 requests, the fp32 module's normalised
    pooled features and the same module run in bf16 by PyTorch (the yardstick for 1 - cos). Computed once."""
    cache, models = {}, {}

    def get(arch, image):
        if arch not in models:
            models[arch] = _model(arch)
        if (arch, image) not in cache:
            m = models[arch]
            x = torch.randn(4, 3, image, image, generator=torch.Generator().manual_seed(image))
            with torch.no_grad():
                ref = V.pool_norm_ref(m.features(x), True)
                mb = registry.get(arch).make_model().eval()
                mb.load_state_dict(m.state_dict())
                yard = V.pool_norm_ref(mb.to(torch.bfloat16).features(x.to(torch.bfloat16)).float(), True)
            cache[arch, image] = m.state_dict(), x, ref, yard
        return cache[arch, image]

    return get


def _engine_rows(out, ref, yard, what):
    """1 - cos <= 4 * max(d16, 2e-5) per image: the margin and floor tests/test_embed_gpu.py applies."""
    for b in range(out.shape[0]):
        d, d16 = float(1 - _cos(out[b:b + 1], ref[b:b + 1])), float(1 - _cos(yard[b:b + 1], ref[b:b + 1]))
        print(f"{what} row {b}: 1-cos {d:.3e}  (bf16 PyTorch {d16:.3e})  | ||v|| - 1 | {abs(float(out[b].double().norm()) - 1):.2e}")
        assert d <= 4 * max(d16, 2e-5)


ENGINES = [("resnet18", 224, 1), ("resnet18", 224, 4), ("resnet50", 224, 1), ("resnet50", 224, 4),
           ("resnet50", 64, 1), ("resnet50", 32, 1)]


@pytest.mark.parametrize("arch,image,batch", ENGINES)
def test_embedding_engine_matches_the_torch_module(nets, arch, image, batch):
    sd, x, ref, yard = nets(arch, image)
    dim = 512 if arch == "resnet18" else 2048
    eng = Engine.from_state_dict(arch, sd, DEV, batch=batch,
                                 arch_kw={"head": "embed", "normalize": True, "image": image})
    assert eng.embed == {"pooling": "mean", "normalize": True, "dim": dim}
    tails = [f for f in eng.contexts[0].fused.values() if f.kind == "tail"]
    # the tail seam binds for the bottleneck net down to 2 pixels; at 1 pixel (image 32) the blocked path runs
    assert len(tails) == int(arch == "resnet50" and image > 32)
    out = eng.infer(x[:batch])
    assert out.shape == (batch, dim) and out.dtype == torch.float32 and torch.isfinite(out).all()
    _engine_rows(out, ref[:batch], yard[:batch], f"{arch} image {image} batch {batch}")
    assert ((out.double().norm(dim=1) - 1).abs() <= dim * 2.0 ** -23).all()


def test_unfused_tail_agrees_with_the_fused_one(nets, monkeypatch):
    sd, x, ref, yard = nets("resnet50", 224)
    kw = {"head": "embed", "normalize": True}
    fused = Engine.from_state_dict("resnet50", sd, DEV, batch=1, arch_kw=kw)
    monkeypatch.setenv("HIPZAP_FUSE", ",".join(k for k in fusion.DEFAULT.split(",") if k != "tail"))
    plain = Engine.from_state_dict("resnet50", sd, DEV, batch=1, arch_kw=kw)
    monkeypatch.undo()
    kf = sorted(f.kind for f in fused.contexts[0].fused.values())
    kp = sorted(f.kind for f in plain.contexts[0].fused.values())
    assert "tail" in kf and "tail" not in kp and [k for k in kf if k != "tail"] == kp
    a, b = fused.infer(x[:1]), plain.infer(x[:1])
    d, d16 = float(1 - _cos(a, b)), float(1 - _cos(yard[:1], ref[:1]))
    print(f"fused vs unfused tail: 1-cos {d:.3e}  (bf16 PyTorch against fp32 {d16:.3e})")
    assert d <= 4 * max(d16, 2e-5)
    _engine_rows(b, ref[:1], yard[:1], "resnet50 image 224 batch 1, tail unfused")


# ---------------------------------------------------------------- program and graph
@pytest.fixture(scope="module")
def r50(tmp_path_factory):
    """ResNet-50 packed on the CPU (what a plan holds), the same parameters on the device, its checkpoint."""
    from hipzap.parallel.comm import _rebuild, _tensor_fields
    m = _model("resnet50")
    root = tmp_path_factory.mktemp("r50emb")
    ckpt = str(root / "r50.pth")
    torch.save(m.state_dict(), ckpt)
    params, kw = registry.get("resnet50").pack(m.state_dict(), "cpu")
    dev = torch.device(DEV)
    p_dev = {k: _rebuild(v, {n: t.to(dev) for n, t in _tensor_fields(v)}) for k, v in params.items()}
    return m, root, ckpt, params, p_dev, kw


def _kinds(g, params, **kw):
    rec = P.PlanRecorder()
    ExecContext(g, params, torch.device("cpu"), None, host_io=True, zero_copy="all", lib=rec, **kw)
    return [arg for t, arg, _, _ in rec.ops if t == P.OP_KERNEL]


def test_embedding_program_is_the_classifiers_with_kind_38_for_13(r50):
    _, _, _, params, p_dev, kw = r50
    gc = build_graph("resnet50", 1, 1000, 224, True)
    ge = build_graph("resnet50", 1, 1000, 224, True, head="embed")
    for fuse in (None, fusion.DEFAULT + ",stem"):  # a pinned request (29 launches), a device-resident one (28)
        kc, ke = _kinds(gc, params, fuse=fuse), _kinds(ge, params, fuse=fuse)
        assert len(kc) == len(ke) == (28 if fuse else 29)
        assert kc.count(N.HZ_K_POOL_FC) == 1 and kc[-1] == N.HZ_K_POOL_FC and N.HZ_K_POOL_NORM not in kc
        assert ke == [N.HZ_K_POOL_NORM if k == N.HZ_K_POOL_FC else k for k in kc]
    # and as bound on the device: the same number of ops, the reader bound on the channel means
    ec = Engine("resnet50", p_dev, DEV, batch=1, arch_kw=dict(kw, input_uint8=True), zero_copy="all")
    ee = Engine("resnet50", p_dev, DEV, batch=1, arch_kw=dict(kw, input_uint8=True, head="embed"), zero_copy="all")
    assert ec.contexts[0].num_ops() == ee.contexts[0].num_ops()
    assert [c[1] for c in ec.contexts[0].configs] == [c[1] for c in ee.contexts[0].configs]
    assert len(ee.contexts[0].pooled_readers) == 1


def test_classification_graph_is_the_parents():
    """``build_graph("resnet50", 1)`` node for node and tensor for tensor against the recording of the commit
    before the embedding head (tests/golden/resnet50_bs1_graph.json: kinds, wiring, slots, attrs, shapes)."""
    want = json.load(open(GOLDEN))
    g = build_graph("resnet50", 1)

    def enc(v):
        return list(v) if isinstance(v, tuple) else v
    assert (g.name, g.inputs, g.outputs) == (want["name"], want["inputs"], want["outputs"])
    assert [[list(t.shape), str(t.dtype).replace("torch.", ""), t.name, bool(t.external)] for t in g.tensors] == \
        want["tensors"]
    assert [[n.kind, list(n.inputs), list(n.outputs), n.slot, {k: enc(v) for k, v in sorted(n.attrs.items())}]
            for n in g.nodes] == want["nodes"]
    assert len(g.nodes) == 56 and not (getattr(g, "meta", None) or {})


# ---------------------------------------------------------------- plans
RZ = (256, 224, 512, 512)


def _u8(h, w, seed):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def plans(r50):
    _, _, ckpt, _, _, _ = r50
    emb = {"pooling": "mean", "normalize": True}
    fixed = P.export_from_checkpoint("resnet50", ckpt, embed=emb)
    rz = P.export_from_checkpoint("resnet50", ckpt, embed=emb, resize=RZ)
    assert (fixed, rz) == (ckpt + ".emb.hzplan", ckpt + ".emb.rz.hzplan")
    return fixed, rz


def test_fixed_shape_embedding_plan_serves_the_engines_bits(r50, plans, monkeypatch):
    """The plan binds its request in pinned host memory, so the torch-built engine is held to the same
    (``HIPZAP_REQSLOT=host``): both programs are then the same launches with the same untuned default
    configs over the same packed bytes, and no tolerance applies. Eager first request, then captured."""
    from hipzap.lite import PlanEngine, read_meta
    from hipzap.serve.server import PlanVisionBackend
    from hipzap.serve.settings import ModelSpec
    _, _, _, _, p_dev, kw = r50
    fixed, _ = plans
    assert read_meta(fixed)["embed"] == {"pooling": "mean", "normalize": True, "dim": 2048}
    monkeypatch.setenv("HIPZAP_REQSLOT", "host")
    eng = Engine("resnet50", p_dev, DEV, batch=1, num_contexts=1, host_io=True, zero_copy="all",
                 arch_kw=dict(kw, input_uint8=True, head="embed", pooling="mean", normalize=True))
    monkeypatch.undo()
    be = PlanVisionBackend("resnet50", fixed, 0, ModelSpec(name="resnet50"))
    assert be.embed == {"pooling": "mean", "normalize": True, "dim": 2048} and be.resize is None
    imgs = torch.stack([_u8(224, 224, s) for s in (1, 2)]).numpy()
    eager = be.embed_u8(imgs)  # the first request of a lazily captured plan runs launch by launch
    be.engine.ensure_contexts()
    replay = be.embed_u8(imgs)
    assert eager.shape == (2, 2048) and eager.dtype == np.float32 and np.isfinite(eager).all()
    assert np.array_equal(eager.view(np.int32), replay.view(np.int32))
    want = torch.cat([eng.infer(torch.from_numpy(imgs[i:i + 1])) for i in range(2)]).numpy()
    assert np.array_equal(want.view(np.int32), replay.view(np.int32))
    assert np.abs(np.linalg.norm(replay.astype(np.float64), axis=1) - 1).max() <= 2048 * 2.0 ** -23
    with pytest.raises(ValueError, match="is an embedding plan: POST /embed"):
        be.infer_u8(imgs)
    pe = PlanEngine(fixed, device=0)  # PlanEngine alone: the raw output bytes are the [1, 2048] vector
    raw = np.frombuffer(pe.infer_raw(imgs[:1]), np.float32)
    assert np.array_equal(raw.view(np.int32), want[0].view(np.int32))
    pe.close()


def test_resize_embedding_plan_serves_the_engines_bits(r50, plans):
    from hipzap.lite import PlanEngine
    from hipzap.serve.server import PlanVisionBackend
    from hipzap.serve.settings import ModelSpec
    _, _, _, _, p_dev, kw = r50
    _, rz = plans
    eng = Engine("resnet50", p_dev, DEV, batch=1, num_contexts=1, host_io=True, zero_copy="all",
                 arch_kw=dict(kw, resize=list(RZ), head="embed", pooling="mean", normalize=True))
    assert eng.resize["max_w"] == 512 and eng.embed["dim"] == 2048
    be = PlanVisionBackend("resnet50", rz, 0, ModelSpec(name="resnet50"))
    assert be.resize == {"resize": 256, "crop": 224, "max_h": 512, "max_w": 512} and be.embed["dim"] == 2048
    imgs = [_u8(97, 131, 3).numpy(), _u8(300, 260, 4).numpy()]
    assert be.accepts_u8((1, 97, 131, 3)) and not be.accepts_u8((1, 600, 8, 3))
    eager = be.embed_u8(imgs)
    be.engine.ensure_contexts()
    replay = be.embed_u8(imgs)
    assert eager.shape == (2, 2048) and np.array_equal(eager.view(np.int32), replay.view(np.int32))
    want = torch.cat([eng.infer_image(torch.from_numpy(im)).reshape(1, -1) for im in imgs]).numpy()
    assert np.array_equal(want.view(np.int32), replay.view(np.int32))
    assert not np.array_equal(replay[0], replay[1])
    pe = PlanEngine(rz, device=0)
    raw = np.frombuffer(pe.infer_image(imgs[1]), np.float32)
    assert np.array_equal(raw.view(np.int32), want[1].view(np.int32))
    pe.close()


# ---------------------------------------------------------------- routes
N_ROWS, DIM = 600, 2048


@pytest.fixture(scope="module")
def served(r50, plans):
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    _, root, _, _, _, _ = r50
    fixed, _ = plans
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((12, DIM)).astype(np.float32)
    rows = centres[rng.integers(0, 12, N_ROWS)] + 0.3 * rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    idx = str(root / "imgs.hzidx")
    S.write_index(idx, rows, "cosine", model="resnet50", embed={"pooling": "mean", "normalize": True, "dim": DIM},
                  tags=np.zeros(N_ROWS, np.uint32))
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["r50-emb"] = ModelSpec(name="resnet50", key="r50.pth",
                                     extra={"embed": True, "plan": fixed, "index": idx, "index_writable": True,
                                            "index_reserve": 64})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv
    srv.close()
    app_mod.set_server(None)


def _img_body(img, **kw):
    return dict({"model": "r50-emb", "image_b64": base64.b64encode(img.tobytes()).decode(), "shape": list(img.shape)}, **kw)


def test_embed_route_with_an_image_body(served):
    from hipzap.serve.server import PlanVisionBackend
    c, srv = served
    img = _u8(224, 224, 11).numpy()
    r = c.post("/embed", json=_img_body(img))
    assert r.status_code == 200, r.data
    j = r.json
    assert (j["model"], j["backend"], j["batch"], j["dim"], j["pooling"], j["normalized"]) == \
        ("r50-emb", "gpu", 1, 2048, "mean", True)
    e = np.asarray(j["embeddings"], np.float32)
    rb = c.post("/embed", json=_img_body(img), headers={"Accept": "application/octet-stream"})
    a = np.load(io.BytesIO(rb.data), allow_pickle=False)
    assert rb.status_code == 200 and a.dtype == np.float32 and a.shape == (1, 2048) and np.array_equal(a, e)
    assert abs(float(np.linalg.norm(a.astype(np.float64))) - 1) <= 2048 * 2.0 ** -23
    backend = srv.vision("r50-emb")
    assert isinstance(backend, PlanVisionBackend) and backend._torch is None
    r = c.post("/predict", json=_img_body(img))
    assert r.status_code == 400 and "is an embedding plan: POST /embed" in r.json["message"], r.data


def test_index_add_then_search_with_image_bodies(served):
    c, srv = served
    img, other = _u8(224, 224, 12).numpy(), _u8(224, 224, 13).numpy()
    r = c.post("/index/add", json=_img_body(img, tags=[5]))
    assert r.status_code == 200, r.data
    assert r.json["ids"] == [N_ROWS] and r.json["count"] == N_ROWS + 1
    index = srv.index("r50-emb", srv.vision("r50-emb"))
    assert isinstance(index, S.Index) and (index.dim, index.metric) == (DIM, "cosine")
    for body_img in (img, other):
        vec = np.load(io.BytesIO(c.post("/embed", json=_img_body(body_img),
                                        headers={"Accept": "application/octet-stream"}).data), allow_pickle=False)
        r = c.post("/search", json=_img_body(body_img, k=5), headers={"Accept": "application/octet-stream"})
        assert r.status_code == 200, r.data
        got = np.load(io.BytesIO(r.data), allow_pickle=False)
        scores, ids = index.search(S.normalize_rows(vec), 5)
        assert np.array_equal(got["id"], ids) and np.array_equal(got["score"].view(np.int32), scores.view(np.int32))
        assert len(set(got["id"][0])) == 5
        if body_img is img:  # the added image's row is its own vector rounded to bf16: its nearest neighbour
            assert got["id"][0, 0] == N_ROWS
    j = c.post("/search", json=_img_body(img, k=3)).json
    assert j["results"][0][0]["id"] == N_ROWS and abs(j["results"][0][0]["score"] - 1.0) <= 2.0 ** -8 + 1e-4
    assert j["results"][0][0]["score"] > j["results"][0][1]["score"]
    j = c.post("/search", json=_img_body(img, k=3, tag=5)).json  # only the added row carries tag 5
    assert [h["id"] for h in j["results"][0]] == [N_ROWS, -1, -1]
