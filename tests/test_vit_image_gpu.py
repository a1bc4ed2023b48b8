"""ViT resize plans on MI355X: the fused resize + patchify kernel against its fp32 oracle and, bit for
bit, against the NHWC8 resize kernel; crop sizes from one patch (240 idle threads) to every thread
live; batch indexing; the launcher's refusals; the kernel as the first launch of a 2-layer ViT-B/16 --
torch engine, plan engine (bitwise equal) -- and ``POST /embed`` / ``POST /predict`` with a PNG."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap.engine.engine import Engine
from hipzap.engine.plan import export_from_checkpoint
from hipzap.engine.reference import run_graph_reference
from hipzap.lite import PlanEngine, PlanError, read_meta
from hipzap.models import vit
from hipzap.ops import vision as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(224, 224), (375, 500), (97, 131), (64, 48), (1, 1), (1024, 1024)]
MAX = (1024, 1024)
RZ = (256, 224, 512, 512)  # the model tests' plan: resize 256, crop 224, images up to 512 x 512
NORM = dict(mean=V.IMAGENET_MEAN, std=V.IMAGENET_STD)


def _image(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _pack(imgs, resize=256, crop=224, fill=None):
    buf, dims = V.pack_images(imgs, resize, crop, *MAX)
    if fill is not None:  # random bytes everywhere beyond each image
        for i, im in enumerate(imgs):
            buf[i, im.numel():] = fill[i, im.numel():]
    return buf.to(DEV), dims.to(DEV)


def _rows(imgs, resize=256, crop=224, fill=None, out=None):
    buf, dims = _pack(imgs, resize, crop, fill)
    y = V.resize_patchify(buf, dims, crop, *MAX, out=out, **NORM)
    torch.cuda.synchronize()
    return y.cpu()


def _check_oracle(got, imgs, resize, crop):
    """|got - y| <= 2^-8 |y| + 1e-4: round-to-nearest bf16's half ulp plus fp32 summation noise."""
    want = V.resize_patchify_reference(imgs, resize=resize, crop=crop)
    assert got.shape == want.shape == (len(imgs) * (crop // 16) ** 2, 768)
    err = (got.float() - want).abs()
    bound = 2.0 ** -8 * want.abs() + 1e-4
    print([tuple(i.shape[:2]) for i in imgs], "crop", crop, "max err", err.max().item(), "max err/bound",
          (err / bound).max().item())
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("hw", SHAPES)
def test_kernel_matches_oracle(hw):
    img = _image(*hw, seed=hw[0] + 3 * hw[1])
    _check_oracle(_rows([img]), [img], 256, 224)


@pytest.mark.parametrize("hw", SHAPES)
def test_bitwise_equal_to_the_nhwc8_kernel(hw):
    """rows[(py * 14 + px), c * 256 + ky * 16 + kx] has the bits of nhwc[py * 16 + ky, px * 16 + kx, c]."""
    img = _image(*hw, seed=hw[0] + 3 * hw[1])
    buf, dims = _pack([img])
    rows = V.resize_patchify(buf, dims, 224, *MAX, **NORM)
    nhwc = V.resize_preprocess(buf, dims, 224, *MAX, **NORM)
    torch.cuda.synchronize()
    want = nhwc[0, :, :, :3].reshape(14, 16, 14, 16, 3).permute(0, 2, 4, 1, 3).reshape(196, 768).contiguous()
    assert torch.equal(rows.view(torch.int16).cpu(), want.view(torch.int16).cpu())


@pytest.mark.parametrize("crop,hw", [(16, (50, 70)), (32, (50, 70)), (240, (50, 70)), (256, (50, 70)),
                                     (256, (300, 260))])
def test_crop_sizes(crop, hw):
    """Crop 16: one patch, 48 chunks, 240 threads without a pixel; 256: every thread owns a column. The
    small crops write into a buffer with 4 KiB of sentinel on each side, which must stay untouched."""
    img = _image(*hw, seed=crop + hw[0])
    if crop > 32:
        _check_oracle(_rows([img], crop, crop), [img], crop, crop)
        return
    n, guard = (crop // 16) ** 2 * 768, 2048  # bf16 elements
    flat = torch.empty(n + 2 * guard, dtype=torch.bfloat16, device=DEV)
    flat.view(torch.int16).fill_(0x5A5A)
    got = _rows([img], crop, crop, out=flat[guard: guard + n]).reshape(-1, 768)
    _check_oracle(got, [img], crop, crop)
    bits = flat.view(torch.int16).cpu()
    assert (bits[:guard] == 0x5A5A).all() and (bits[guard + n:] == 0x5A5A).all()


def test_batch_rows_use_their_own_header_and_only_their_image():
    a, b = _image(375, 500, seed=1), _image(130, 97, seed=2)
    both = _rows([a, b])
    assert both.shape == (392, 768)
    assert torch.equal(both[:196], _rows([a])) and torch.equal(both[196:], _rows([b]))
    assert not torch.equal(both[:196], both[196:])
    img = _image(97, 131, seed=4)
    cap = V.resize_cap_bytes(*MAX)
    fills = [torch.randint(0, 256, (1, cap), dtype=torch.uint8, generator=torch.Generator().manual_seed(s))
             for s in (10, 11)]
    assert torch.equal(_rows([img], fill=fills[0]), _rows([img], fill=fills[1]))


def test_launcher_refusals():
    """Host-side argument checks: nothing is launched."""
    buf, dims = _pack([_image(50, 70)])
    out = torch.zeros(256 * 768 + 8, dtype=torch.bfloat16, device=DEV)

    def launch(crop, out_ptr):
        prm = V.resize_params(buf.data_ptr(), dims.data_ptr(), out_ptr, 1, crop, *MAX, **NORM)
        N.check(N.lib().hz_launch_kernel(N.HZ_K_RESIZE_PATCHIFY, C.byref(prm), N.stream_ptr()), "resize_patchify")

    for crop in (230, 272, 8):
        with pytest.raises(RuntimeError, match="resize_patchify failed with code -1"):
            launch(crop, out.data_ptr())
    with pytest.raises(RuntimeError, match="resize_patchify failed with code -1"):
        launch(224, out.data_ptr() + 8)
    torch.cuda.synchronize()
    assert (out == 0).all()


# ---------------------------------------------------------------- a 2-layer ViT-B/16 behind the kernel
@pytest.fixture(scope="module")
def vit2(tmp_path_factory):
    from hipzap.parallel.comm import _rebuild, _tensor_fields
    torch.manual_seed(0)
    sd = vit.make_model(num_hidden_layers=2).state_dict()
    ckpt = str(tmp_path_factory.mktemp("vitrz") / "vit2.pth")
    torch.save(sd, ckpt)
    params, kw = vit.pack_vit(sd, "cpu")
    kw = dict(kw, resize=list(RZ))
    path = export_from_checkpoint("vit-b16", ckpt, resize=RZ)
    assert path == ckpt + ".rz.hzplan"
    assert read_meta(path)["resize"] == {"resize": 256, "crop": 224, "max_h": 512, "max_w": 512}
    dev = torch.device(DEV)
    p_dev = {k: _rebuild(v, {n: t.to(dev) for n, t in _tensor_fields(v)}) for k, v in params.items()}
    eng = Engine("vit-b16", p_dev, dev, batch=1, num_contexts=1, arch_kw=kw, host_io=True, zero_copy="all")
    pe = PlanEngine(path, device=0, contexts=2)
    return params, eng, pe, path, ckpt


def _plan_out(pe, img, **kw):
    return np.frombuffer(pe.infer_image(np.asarray(img), **kw), np.float32).copy()


def _rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@pytest.mark.parametrize("hw", [(375, 500), (64, 48)])
def test_resize_plan_logits(vit2, hw):
    params, eng, pe, _, _ = vit2
    assert eng.resize == {"resize": 256, "crop": 224, "max_h": 512, "max_w": 512}
    img = _image(*hw, seed=hw[0])
    y = eng.infer_image(img)
    buf, dims = V.pack_images([img], *RZ)
    ref = run_graph_reference(eng.graph, params, [buf, dims])[eng.graph.outputs[0]].reshape(1, -1)
    err = _rel(y.reshape(1, -1)[:, : ref.shape[1]], ref)
    print(hw, "max-normalised error", err)
    assert err < 5e-2
    yp = _plan_out(pe, img.numpy())
    assert np.array_equal(yp.view(np.int32), y.numpy().reshape(-1).view(np.int32))
    assert np.array_equal(_plan_out(pe, img.numpy(), ctx=1).view(np.int32), yp.view(np.int32))


def test_oversized_image_names_the_limit(vit2):
    _, eng, pe, _, _ = vit2
    with pytest.raises(PlanError, match="512x512"):
        pe.infer_image(np.zeros((8, 600, 3), np.uint8))
    with pytest.raises(ValueError, match="512x512"):
        eng.infer_image(torch.zeros(8, 600, 3, dtype=torch.uint8))


def test_small_image_after_a_large_one(vit2):
    _, _, _, path, _ = vit2
    big, small = _image(500, 375, seed=21), _image(70, 90, seed=22)
    fresh = PlanEngine(path, device=0, contexts=2)
    solo_small = _plan_out(fresh, small.numpy(), ctx=0)  # a context that never held a larger image
    used = _plan_out(fresh, big.numpy(), ctx=1)
    assert not np.array_equal(used, solo_small)
    assert np.array_equal(_plan_out(fresh, small.numpy(), ctx=1), solo_small)


def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def _serve(path, extra):
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    st = Settings(default_model="vit-b16")
    st.models["vit-b16"] = ModelSpec(name="vit-b16", contexts=2, extra=dict(extra, plan=path))
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    return app_mod, srv


def test_embed_png_on_a_resize_embedding_plan(vit2):
    _, _, _, _, ckpt = vit2
    path = export_from_checkpoint("vit-b16", ckpt, resize=RZ, embed={"pooling": "cls", "normalize": True})
    assert path == ckpt + ".emb.rz.hzplan"
    meta = read_meta(path)
    assert meta["embed"] == {"pooling": "cls", "normalize": True, "dim": 768} and meta["resize"]["max_w"] == 512
    app_mod, srv = _serve(path, {"resize": 256, "embed": {"pooling": "cls", "normalize": True}})
    try:
        img = _image(97, 131, seed=30).numpy()
        with app_mod.app.test_client() as c:
            r = c.post("/embed", data=_png(img), content_type="image/png",
                       headers={"Accept": "application/octet-stream"})
            assert r.status_code == 200, r.data
            vec = np.load(io.BytesIO(r.data), allow_pickle=False)
            assert vec.shape == (1, 768) and vec.dtype == np.float32
            want = _plan_out(PlanEngine(path, device=0, contexts=1), img)
            assert np.array_equal(vec.reshape(-1).view(np.int32), want.view(np.int32))
            assert abs(float(np.linalg.norm(vec)) - 1.0) < 1e-3
            backend = srv.vision("vit-b16")
            assert backend.resize is not None and backend._torch is None
            r = c.post("/predict", data=_png(img), content_type="image/png")
            assert r.status_code == 400 and "POST /embed" in r.json["message"], r.data
            r = c.post("/embed", data=_png(np.zeros((8, 600, 3), np.uint8)), content_type="image/png")
            assert r.status_code == 400 and "512x512" in r.json["message"], r.data
            assert backend._torch is None
    finally:
        app_mod.set_server(None)


def test_predict_png_on_a_resize_plan(vit2):
    _, _, pe, path, _ = vit2
    app_mod, srv = _serve(path, {"resize": 256})
    try:
        img = _image(97, 131, seed=31).numpy()
        with app_mod.app.test_client() as c:
            r = c.post("/predict?logits=1", data=_png(img), content_type="image/png")
            assert r.status_code == 200, r.data
            assert r.json["backend"] == "gpu" and r.json["batch"] == 1
            want = _plan_out(pe, img)
            assert r.json["top5"][0][0][0] == int(want[:1000].argmax())
            got = np.asarray(r.json["logits"][0], np.float32)
            assert np.array_equal(got, want[: len(got)])
            r = c.post("/predict", data=_png(np.zeros((8, 600, 3), np.uint8)), content_type="image/png")
            assert r.status_code == 400 and "512x512" in r.json["message"], r.data
            assert srv.vision("vit-b16")._torch is None
    finally:
        app_mod.set_server(None)
