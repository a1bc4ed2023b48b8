"""Resize plans on MI355X: the fused resize + crop + normalise kernel against its fp32 oracle, batch
indexing, reads confined to the image, and the kernel as the first launch of a ResNet-18 program --
torch engine, plan engine (bitwise equal), the executor's sized submit on concurrent contexts, and
``POST /predict`` with a PNG."""
import io
import threading

import numpy as np
import pytest
import torch

from hipzap.engine.engine import Engine
from hipzap.engine.plan import export_plan
from hipzap.engine.reference import run_graph_reference
from hipzap.lite import PlanEngine, PlanError
from hipzap.models import registry
from hipzap.models.resnet import randomize_bn
from hipzap.ops import vision as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(256, 256), (224, 224), (375, 500), (500, 375), (97, 131), (64, 48), (300, 1000), (1, 1), (1024, 768),
          (1024, 1024)]
MAX = (1024, 1024)
RZ = (256, 224, 512, 512)  # the model tests' plan: resize 256, crop 224, images up to 512 x 512


def _image(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _run(imgs, fill=None):
    buf, dims = V.pack_images(imgs, 256, 224, *MAX)
    if fill is not None:  # random bytes everywhere beyond each image
        for i, im in enumerate(imgs):
            buf[i, im.numel():] = fill[i, im.numel():]
    out = V.resize_preprocess(buf.to(DEV), dims.to(DEV), 224, *MAX, mean=V.IMAGENET_MEAN, std=V.IMAGENET_STD)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("hw", SHAPES)
def test_kernel_matches_oracle(hw):
    """|got - y| <= 2^-8 |y| + 1e-4: round-to-nearest bf16's half ulp plus fp32 summation noise; the
    padding channels are exactly zero. (97, 131): rows of 393 bytes, no multiple of 4."""
    img = _image(*hw, seed=hw[0] + 3 * hw[1])
    got = _run([img])[0].float()
    want = V.resize_preprocess_reference(img)
    assert got.shape == want.shape == (224, 224, 8)
    assert (got[..., 3:] == 0).all()
    err = (got[..., :3] - want[..., :3]).abs()
    bound = 2.0 ** -8 * want[..., :3].abs() + 1e-4
    print(hw, "max err", err.max().item(), "max err/bound", (err / bound).max().item())
    assert (err <= bound).all(), (err - bound).max().item()


def test_batch_rows_use_their_own_header():
    a, b = _image(375, 500, seed=1), _image(130, 97, seed=2)
    both = _run([a, b])
    assert torch.equal(both[0], _run([a])[0]) and torch.equal(both[1], _run([b])[0])
    assert not torch.equal(both[0], both[1])


def test_bytes_beyond_the_image_are_never_used():
    img = _image(97, 131, seed=4)
    cap = V.resize_cap_bytes(*MAX)
    fills = [torch.randint(0, 256, (1, cap), dtype=torch.uint8, generator=torch.Generator().manual_seed(s))
             for s in (10, 11)]
    assert torch.equal(_run([img], fills[0]), _run([img], fills[1]))


# ---------------------------------------------------------------- ResNet-18 behind the kernel
@pytest.fixture(scope="module")
def r18(tmp_path_factory):
    from hipzap.parallel.comm import _rebuild, _tensor_fields
    torch.manual_seed(0)
    a = registry.get("resnet18")
    sd = randomize_bn(a.make_model()).eval().state_dict()
    params, kw = a.pack(sd, "cpu")
    kw = dict(kw, resize=list(RZ))
    path = str(tmp_path_factory.mktemp("rzplan") / "r18.rz.hzplan")
    meta = export_plan("resnet18", params, kw, path, batch=1, contexts=1)
    assert meta["resize"] == {"resize": 256, "crop": 224, "max_h": 512, "max_w": 512}
    dev = torch.device(DEV)
    p_dev = {k: _rebuild(v, {n: t.to(dev) for n, t in _tensor_fields(v)}) for k, v in params.items()}
    eng = Engine("resnet18", p_dev, dev, batch=1, num_contexts=1, arch_kw=kw, host_io=True, zero_copy="all")
    pe = PlanEngine(path, device=0, contexts=2)
    return params, eng, pe, path


def _plan_logits(pe, img, **kw):
    return np.frombuffer(pe.infer_image(img.numpy(), **kw), np.float32).copy()


@pytest.mark.parametrize("hw", [(375, 500), (64, 48)])
def test_resize_plan_logits(r18, hw):
    params, eng, pe, _ = r18
    img = _image(*hw, seed=hw[0])
    y = eng.infer_image(img)
    buf, dims = V.pack_images([img], *RZ)
    ref = run_graph_reference(eng.graph, params, [buf, dims])[eng.graph.outputs[0]].reshape(1, -1)
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    print(hw, "max-normalised error", err)
    assert err < 3e-2
    yp = _plan_logits(pe, img)
    assert np.array_equal(yp, y.numpy().reshape(-1)), np.abs(yp - y.numpy().reshape(-1)).max()
    assert np.array_equal(_plan_logits(pe, img, ctx=1), yp)  # the direct (no executor) path, second context


def test_oversized_image_names_the_limit(r18):
    _, eng, pe, _ = r18
    with pytest.raises(PlanError, match="512x512"):
        pe.infer_image(np.zeros((8, 600, 3), np.uint8))
    with pytest.raises(ValueError, match="512x512"):
        eng.infer_image(torch.zeros(600, 8, 3, dtype=torch.uint8))


def test_concurrent_sizes_and_no_stale_tail(r18):
    _, _, pe, path = r18
    big, small = _image(500, 375, seed=21), _image(70, 90, seed=22)
    fresh = PlanEngine(path, device=0, contexts=1)
    solo_small = _plan_logits(fresh, small, ctx=0)  # a context that never held a larger image
    solo_big = _plan_logits(fresh, big, ctx=0)
    assert not np.array_equal(solo_small, solo_big)
    # the same context: a smaller image after a larger one (whose bytes are still in the slot's tail)
    assert np.array_equal(_plan_logits(fresh, small, ctx=0), solo_small)
    # two contexts, two request threads, different sizes at once through the executor's sized submit
    assert pe.executor() is not None
    got = {}

    def work(name, img):
        got[name] = [_plan_logits(pe, img) for _ in range(4)]

    th = [threading.Thread(target=work, args=("big", big)), threading.Thread(target=work, args=("small", small))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(np.array_equal(y, solo_big) for y in got["big"])
    assert all(np.array_equal(y, solo_small) for y in got["small"])


def test_predict_png_on_a_resize_plan(r18):
    from PIL import Image
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    _, _, pe, path = r18
    st = Settings(default_model="resnet18")
    st.models["resnet18"] = ModelSpec(name="resnet18", contexts=2, extra={"plan": path, "resize": 256})
    app_mod.set_server(ModelServer(st, backend="gpu"))
    try:
        img = _image(97, 131, seed=30)
        buf = io.BytesIO()
        Image.fromarray(img.numpy()).save(buf, format="PNG")
        with app_mod.app.test_client() as c:
            r = c.post("/predict?logits=1", data=buf.getvalue(), content_type="image/png")
            assert r.status_code == 200, r.data
            assert r.json["backend"] == "gpu" and r.json["batch"] == 1
            want = _plan_logits(pe, img)
            assert r.json["top5"][0][0][0] == int(want.argmax())
            assert np.array_equal(np.asarray(r.json["logits"][0], np.float32), want[: len(r.json["logits"][0])])
            big = io.BytesIO()
            Image.fromarray(np.zeros((8, 600, 3), np.uint8)).save(big, format="PNG")
            r = c.post("/predict", data=big.getvalue(), content_type="image/png")
            assert r.status_code == 400 and "512x512" in r.json["message"], r.data
    finally:
        app_mod.set_server(None)
