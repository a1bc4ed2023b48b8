"""Resize plans without a GPU: the shared geometry, the fp32 oracle against PIL, the lowering of a
resize graph (new first node, conv1 + maxpool still fused, fixed-shape plans untouched), the plan
metadata and CLI, the Flask route on the CPU backend (encoded images, oversize, bad bodies) and the
executor's sized submit under host sanitizers (a stand-alone program)."""
import base64
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from hipzap.engine import fusion
from hipzap.engine.reference import run_graph_reference
from hipzap.models import registry
from hipzap.models.resnet import randomize_bn
from hipzap.ops import vision as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", shutil.which("hipcc") or "/opt/rocm/bin/hipcc")

GEOMETRY = {(375, 500): (256, 341, 16, 58), (500, 375): (341, 256, 58, 16), (97, 131): (256, 345, 16, 60),
            (300, 1000): (256, 853, 16, 314), (683, 1024): (256, 383, 16, 80), (64, 48): (341, 256, 58, 16),
            (256, 256): (256, 256, 16, 16)}


def _image(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_resize_geometry_table():
    for hw, want in GEOMETRY.items():
        assert V.resize_geometry(*hw) == want, hw
    assert V.resize_dims(375, 500, max_h=512, max_w=512) == [375, 500, 256, 341, 16, 58, 0, 0]
    with pytest.raises(ValueError, match="512x512"):
        V.resize_dims(375, 600, max_h=512, max_w=512)


@pytest.mark.parametrize("hw", sorted(GEOMETRY))
def test_oracle_agrees_with_pil(hw):
    """PIL's BILINEAR resize (what torchvision runs on PIL inputs) rounds to 8 bits after each of its
    two passes: at most 1.01 grey levels from the fp32 oracle, i.e. 1.01 / (255 * std_c) after the
    normalisation."""
    from PIL import Image
    img = _image(*hw, seed=hw[0] * 7 + hw[1])
    rh, rw, top, left = V.resize_geometry(*hw)
    pil = np.asarray(Image.fromarray(img.numpy()).resize((rw, rh), Image.BILINEAR))[top: top + 224, left: left + 224]
    want = (pil.astype(np.float32) / 255.0 - np.asarray(V.IMAGENET_MEAN, np.float32)) / np.asarray(V.IMAGENET_STD,
                                                                                                  np.float32)
    got = V.resize_preprocess_reference(img)
    assert got.shape == (224, 224, 8) and (got[..., 3:] == 0).all()
    err = np.abs(got[..., :3].numpy() - want).reshape(-1, 3).max(0)
    bound = 1.01 / (255.0 * np.asarray(V.IMAGENET_STD))
    print(hw, "grey levels", err * 255.0 * np.asarray(V.IMAGENET_STD))
    assert (err <= bound).all(), (err, bound)


@pytest.fixture(scope="module")
def r18():
    torch.manual_seed(0)
    a = registry.get("resnet18")
    params, kw = a.pack(randomize_bn(a.make_model()).eval().state_dict(), "cpu")
    return a, params, kw


def test_resize_graph_lowering(r18):
    a, params, kw = r18
    g = a.build_graph(batch=1, **kw, resize=(256, 224, 512, 512))
    assert g.nodes[0].kind == "resize_preprocess" and not any(n.kind == "preprocess" for n in g.nodes)
    assert [g.shape(t) for t in g.inputs] == [(1, 512 * 512 * 3), (1, 8)]
    for kinds in (None, set(fusion.KINDS)):  # the default set, and every fusion enabled
        kinds_found = {f.kind for f in fusion.plan(g, params, kinds).values()}
        assert "convpool" in kinds_found and "stem" not in kinds_found
    img = _image(375, 500, seed=3)
    buf, dims = V.pack_images([img], 256, 224, 512, 512)
    assert dims.tolist() == [[375, 500, 256, 341, 16, 58, 0, 0]]
    got = run_graph_reference(g, params, [buf, dims])[g.outputs[0]]
    # the fixed-shape sibling fed the oracle's tensor: an fp32 NCHW graph without normalisation
    sib = a.build_graph(batch=1, **kw)
    x = V.resize_preprocess_reference(img)[..., :3].permute(2, 0, 1)[None].contiguous()
    want = run_graph_reference(sib, params, [x])[sib.outputs[0]]
    assert torch.equal(got, want)


def test_fixed_shape_resnet50_still_matches_stem():
    torch.manual_seed(0)
    a = registry.get("resnet50")
    with torch.device("meta"):
        m = a.make_model()
    from hipzap.models.resnet import pack_resnet
    params = pack_resnet(m.state_dict(), "meta")
    g = a.build_graph(batch=1, input_uint8=True)
    assert fusion.plan(g, params, set(fusion.KINDS))[0].kind == "stem"
    assert fusion.plan(g, params)[1].kind == "convpool"  # the default set: standalone preprocess + convpool


def test_plan_cli_resize_lands_in_meta(tmp_path, r18):
    from hipzap.__main__ import main
    from hipzap.engine.plan import export_plan
    from hipzap.lite import read_meta
    a, params, kw = r18
    torch.manual_seed(0)
    ckpt = str(tmp_path / "r18.pth")
    torch.save(randomize_bn(a.make_model()).eval().state_dict(), ckpt)
    main(["plan", "--model", "resnet18", "--ckpt", ckpt, "--resize", "256", "--max-image", "320x384"])
    meta = read_meta(ckpt + ".rz.hzplan")
    assert meta["resize"] == {"resize": 256, "crop": 224, "max_h": 320, "max_w": 384}
    assert [i["shape"] for i in meta["inputs"]] == [[1, 320 * 384 * 3], [1, 8]]
    assert [i["dtype"] for i in meta["inputs"]] == ["uint8", "int32"]
    main(["plan", "--model", "resnet18", "--ckpt", ckpt, "--resize", "256", "--out", str(tmp_path / "d.hzplan")])
    assert read_meta(str(tmp_path / "d.hzplan"))["resize"]["max_h"] == 1024  # default maximum 1024 x 1024
    # a plan without --resize: no "resize" key, the fixed-shape inputs as before
    fixed = str(tmp_path / "fixed.hzplan")
    export_plan("resnet18", params, dict(kw, input_uint8=True), fixed, batch=1)
    fm = read_meta(fixed)
    assert "resize" not in fm and fm["inputs"][0]["shape"] == [1, 224, 224, 3]


def test_settings_extra_resize():
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    st = Settings(default_model="resnet18")
    st.models["resnet18"] = ModelSpec(name="resnet18", extra={"resize": {"resize": 256, "max_image": "300x400"}})
    st.models["resnet50"] = ModelSpec(name="resnet50", extra={"resize": 288})
    srv = ModelServer(st, backend="cpu")
    assert srv.resize_spec("resnet18") == (256, 224, 300, 400)
    assert srv.resize_spec("resnet50") == (288, 224, 1024, 1024)
    assert srv.resize_spec("vit-b16") == (256, 224, 1024, 1024)


# ---------------------------------------------------------------- the app on the CPU backend
@pytest.fixture(scope="module")
def client():
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import Settings
    mp = pytest.MonkeyPatch()
    mp.setenv("HIPZAP_RANDOM_WEIGHTS", "1")
    app_mod.set_server(ModelServer(Settings(default_model="resnet18"), backend="cpu"))
    with app_mod.app.test_client() as c:
        yield c
    app_mod.set_server(None)
    mp.undo()


def _encode(arr, fmt):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format=fmt)
    return buf.getvalue()


def test_png_body_equals_raw_pixels(client):
    img = _image(97, 131, seed=5).numpy()
    r_png = client.post("/predict?logits=1", data=_encode(img, "PNG"), content_type="image/png")
    r_raw = client.post("/predict?logits=1", json={"image_b64": base64.b64encode(img.tobytes()).decode(),
                                                   "shape": [97, 131, 3]})
    r_json = client.post("/predict?logits=1", json={"image": base64.b64encode(_encode(img, "PNG")).decode()})
    assert r_png.status_code == r_raw.status_code == r_json.status_code == 200, (r_png.data, r_raw.data)
    for key in ("model", "backend", "batch", "top5", "logits"):
        assert r_png.json[key] == r_raw.json[key] == r_json.json[key], key
    assert r_png.json["backend"] == "cpu" and len(r_png.json["top5"][0]) == 5


def test_jpeg_body(client):
    img = _image(120, 90, seed=6).numpy()
    r = client.post("/predict", data=_encode(img, "JPEG"), content_type="image/jpeg")
    assert r.status_code == 200 and len(r.json["top5"][0]) == 5, r.data


def test_oversized_image_is_400_naming_the_limit(client):
    img = np.zeros((8, 1100, 3), np.uint8)
    r = client.post("/predict", data=_encode(img, "PNG"), content_type="image/png")
    assert r.status_code == 400 and "1024x1024" in r.json["message"], r.data


def test_non_image_body_is_400(client):
    r = client.post("/predict", data=b"this is not a png", content_type="image/png")
    assert r.status_code == 400 and r.json["error"] == "ValueError", r.data


def test_lambda_event_with_jpeg_reaches_the_route(client):
    """API Gateway delivers binary bodies base64-encoded; the adapter hands the route the bytes."""
    from hipzap.serve import lambda_handler as LH
    img = _image(80, 100, seed=8).numpy()
    event = {"httpMethod": "POST", "path": "/predict", "headers": {"Content-Type": "image/jpeg"},
             "queryStringParameters": None, "isBase64Encoded": True,
             "body": base64.b64encode(_encode(img, "JPEG")).decode()}
    resp = LH.lambda_handler(event, None)
    assert resp["statusCode"] == 200, resp
    body = base64.b64decode(resp["body"]) if resp["isBase64Encoded"] else resp["body"]
    assert len(json.loads(body)["top5"][0]) == 5


# ---------------------------------------------------------------- executor: sized submit
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_executor_sized_submit_host_sanitizers(tmp_path, sanitizer):
    """hz_exec_submit_sized copies only nbytes[k] (the payloads live in exact-size heap blocks, so a
    copy of the whole pinned input is an ASan report), leaves the rest of the slot as it was, and
    rejects nbytes > in_bytes and dynamic-batching executors."""
    exe = tmp_path / f"exec_sized_{sanitizer.split(',')[0]}"
    san = []
    for f in (f"-fsanitize={sanitizer}", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"):
        san += ["-Xarch_host", f]
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", *san, "-I", os.path.join(ROOT, "hipzap", "csrc"),
           os.path.join(ROOT, "hipzap", "csrc", "executor.cpp"),
           os.path.join(ROOT, "tests", "native", "executor_sized_sanitize.cpp"), "-lpthread", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "executor sized sanitize: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])
    for marker in ("ERROR: AddressSanitizer", "runtime error", "WARNING: ThreadSanitizer"):
        assert marker not in run.stderr, run.stderr[-4000:]
