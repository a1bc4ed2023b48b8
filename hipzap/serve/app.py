"""Flask WSGI application — the Zappa ``app_function`` (``main.app``).

Routes (reference: /root/reference/main.py:17-18, 105-112):
  GET  /inference   AWD-LSTM text generation -> {"response": {"text": str}}   (parity, P3)
                    optional query: prompt, words, seed
  POST /predict     image / tensor classification -> {"model", "top5", "timing_ms", ...}
                    (north-star API; ``model`` selects resnet50 (default), resnet18, ...)
  POST /embed       one pooled vector per text / image from a BERT or ViT encoder served with
                    ``extra.embed`` -> {"model", "dim", "pooling", "normalized", "embeddings", ...}, or a
                    float32 ``.npy`` [n, dim] with ``Accept: application/octet-stream``
  POST /index/add, /index/delete, /index/save   mutate the model's index (``extra.index_writable: true``)
  POST /index/neighbors   nearest live rows of stored rows of the model's index: {"model", "ids", "k"?, "include_self"?}
  POST /search      nearest rows of the model's vector index (``extra.index``, a ``.hzidx`` file) for the
                    bodies of /embed or ready ``vectors`` -> {"model", "metric", "k", "count", "results", ...},
                    or a structured ``.npy`` [Q, k] (id, score) with ``Accept: application/octet-stream``
  GET  /health      liveness + loaded models;  GET /metrics  Prometheus text;  GET /  info
torch is imported lazily: a plan-backed vision model (server.PlanVisionBackend) serves uint8
images end to end without it (decode -> pinned input -> hipGraph -> top-5 in numpy).
CORS is applied to every route and origin (main.py:18 used flask_cors, which is not
installed here: implemented in-house — ``Access-Control-Allow-Origin: *`` plus preflight).
"""
from __future__ import annotations

import base64
import io
import json
import logging
import sys
import time

import numpy as np
from flask import Flask, Response, g, request

from .. import __version__
from ..utils.metrics import METRICS
from ..utils.tracing import PhaseTimer, trace_range
from .server import ModelServer
from .settings import load_settings

log = logging.getLogger("hipzap.app")

app = Flask("hipzap")
_server: ModelServer | None = None
# DP cluster worker state (serve/cluster.py): batched uint8 requests for the DP model are
# scattered over every GPU of the node through the cluster's control plane
CLUSTER: dict = {}
_DP = {"member": None, "model": None, "item_shape": None}


def set_dp(member, model: str | None, item_shape) -> None:
    _DP.update(member=member, model=model, item_shape=tuple(item_shape) if item_shape else None)


def serve_threaded() -> bool:
    """Threaded WSGI serving for the GPU backend (engines take concurrent requests on their own
    contexts/streams). The CPU backend serves on the main thread: eager PyTorch CPU inference
    called from a WSGI worker thread ran 3.5x slower than from the main thread here (OpenMP /
    oneDNN thread handling; 72-77 ms vs 20 ms per ResNet-18 forward), and the eager AWD-LSTM is
    not reentrant anyway."""
    return get_server().backend != "cpu"


def get_server() -> ModelServer:
    global _server
    if _server is None:
        _server = ModelServer(load_settings())
    return _server


def set_server(server: ModelServer | None) -> None:
    global _server
    _server = server


def _json(obj, status=200) -> Response:
    return Response(response=json.dumps(obj), status=status, mimetype="application/json")


def phase(name: str):
    """Time a request phase: roctx range + the request's ``X-Timing`` header entry."""
    return trace_range(name, getattr(g, "hz_timer", None))


@app.after_request
def _cors(resp: Response) -> Response:
    resp.headers["Access-Control-Allow-Origin"] = "*"
    timer = getattr(g, "hz_timer", None)
    t0 = getattr(request, "_hz_t0", None)
    if timer is not None and t0 is not None:  # per-request phase timers (SURVEY.md §5 tracing)
        timer.add("total", (time.perf_counter() - t0) * 1e3)
        resp.headers["X-Timing"] = timer.header()
        resp.headers["Access-Control-Expose-Headers"] = "X-Timing"
    if request.method == "OPTIONS":
        resp.headers["Access-Control-Allow-Methods"] = "GET, POST, OPTIONS"
        req_h = request.headers.get("Access-Control-Request-Headers")
        resp.headers["Access-Control-Allow-Headers"] = req_h or "Content-Type"
        resp.headers["Access-Control-Max-Age"] = "600"
    return resp


@app.before_request
def _preflight():
    request._hz_t0 = time.perf_counter()
    g.hz_timer = PhaseTimer()
    if request.method == "OPTIONS":
        return Response(status=200)
    return None


@app.teardown_request
def _count(exc):
    t0 = getattr(request, "_hz_t0", None)
    if t0 is not None:
        METRICS.observe("hipzap_request_seconds", time.perf_counter() - t0, {"path": request.path})
    METRICS.inc("hipzap_requests_total", {"path": request.path})
    if exc is not None:
        METRICS.inc("hipzap_errors_total", {"path": request.path})


@app.errorhandler(Exception)
def _error(e):
    code = getattr(e, "code", 400 if isinstance(e, ValueError) else 500)  # bad input: client error
    if not isinstance(code, int):
        code = 500
    if code >= 500:
        log.exception("request failed")
    METRICS.inc("hipzap_errors_total", {"path": request.path})
    return _json({"error": type(e).__name__, "message": str(e)}, status=code)


@app.route("/", methods=["GET"])
def index():
    s = get_server()
    return _json({"service": "hipzap", "version": __version__, "backend": s.backend,
                  "routes": ["GET /inference", "POST /predict", "POST /embed", "POST /search", "POST /index/neighbors", "POST /index/add", "POST /index/delete",
                             "POST /index/save", "GET /health", "GET /metrics"]})


@app.route("/inference", methods=["GET"])
def inference():
    """GET: perform inference on the language model (main.py:105-112)."""
    s = get_server()
    prompt = request.args.get("prompt")
    words = [""] if not prompt else prompt.split()
    n = int(request.args.get("words", s.settings.lm_words))
    seed = request.args.get("seed")
    with phase("load"):
        lm = s.lm()
    with phase("generate"):
        text = lm.generate(words, n, seed=int(seed) if seed is not None else None)
    return _json({"response": {"text": text}})


IMAGE_TYPES = ("image/jpeg", "image/png")


def decode_image(data: bytes):
    """An encoded image file (JPEG, PNG, ...) -> uint8 [H, W, 3] RGB array. PIL is imported here, on
    the first such request; without it the answer is 415."""
    try:
        from PIL import Image
    except ImportError:
        from werkzeug.exceptions import UnsupportedMediaType
        raise UnsupportedMediaType("encoded images need Pillow on the server; send image_b64 + shape") from None
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)
    except Exception as e:  # noqa: BLE001 - PIL raises several types for a body that is no image
        raise ValueError(f"request body is not a decodable image: {e}") from None


def decode_input(req):
    """-> (model, numpy array). Accepted request bodies:
    * ``image/jpeg`` / ``image/png``: an encoded image file of any size (decoded with PIL to RGB);
    * JSON ``{"image": base64 of an encoded image file}``: the same;
    * ``application/octet-stream``: a ``.npy`` array (``np.save``; no pickles);
    * JSON ``{"inputs": nested list, "model": ...}`` (float tensor, NCHW or CHW);
    * JSON ``{"image_b64": base64 uint8 HWC bytes, "shape": [H, W, 3]}`` (or [N, H, W, 3]);
    * JSON ``{"tensor_b64": base64 float32 bytes, "shape": [...]}``.
    uint8 arrays are images (HWC / NHWC), served as is by plan-backed models (normalised on
    device; a resize plan takes any size) and normalised to NCHW float for the others
    (:func:`to_model_input`, which first resizes and crops an image of another size on the host)."""
    model = req.args.get("model")
    if req.mimetype in IMAGE_TYPES:
        arr = decode_image(req.get_data())
    elif req.mimetype == "application/octet-stream":
        arr = np.load(io.BytesIO(req.get_data()), allow_pickle=False)
    else:
        body = req.get_json(force=True, silent=False)
        model = body.get("model", model)
        if "image" in body:
            arr = decode_image(base64.b64decode(body["image"]))
        elif "inputs" in body:
            arr = np.asarray(body["inputs"], dtype=np.float32)
        elif "tensor_b64" in body:
            arr = np.frombuffer(base64.b64decode(body["tensor_b64"]), dtype=np.float32).reshape(body["shape"])
        elif "image_b64" in body:
            arr = np.frombuffer(base64.b64decode(body["image_b64"]), dtype=np.uint8).reshape(body["shape"])
        else:
            raise ValueError("request needs one of: image, inputs, tensor_b64, image_b64 (or an image / .npy body)")
    if arr.dtype == np.uint8 and arr.ndim == 3:
        arr = arr[None]
    return model or get_server().settings.default_model, arr


def check_image_size(arr, rz) -> None:
    """ValueError (-> 400) naming the limit for uint8 images above ``rz``'s maximum."""
    _, _, max_h, max_w = rz
    if arr.shape[1] > max_h or arr.shape[2] > max_w:
        raise ValueError(f"image {arr.shape[1]}x{arr.shape[2]} exceeds the maximum of {max_h}x{max_w} "
                         f"(height x width) this model is served with")


def to_model_input(arr, rz=None):
    """numpy request array -> float32 NCHW torch tensor for the torch-built backends. ``rz``
    (resize, crop, max_h, max_w): uint8 images that are not crop x crop already go through the
    resize oracle on the host (ops/vision.py resize_preprocess_reference), the same transform a
    resize plan runs on the GPU."""
    import torch
    if arr.dtype == np.uint8 and rz is not None and arr.ndim == 4 and tuple(arr.shape[1:3]) != (rz[1], rz[1]):
        from ..ops.vision import resize_preprocess_reference
        check_image_size(arr, rz)
        x = torch.stack([resize_preprocess_reference(torch.from_numpy(np.array(a)), resize=rz[0],
                                                     crop=rz[1])[..., :3] for a in arr])
        return x.permute(0, 3, 1, 2).contiguous()
    if arr.dtype == np.uint8:  # NHWC image bytes -> normalised NCHW float
        # in numpy: torch's multi-threaded elementwise ops on this request thread would start an
        # OpenMP team per WSGI thread, spinning against the model's own thread pool
        from ..ops.vision import IMAGENET_MEAN, IMAGENET_STD
        a = (arr.astype(np.float32) * np.float32(1 / 255.0) - np.asarray(IMAGENET_MEAN, np.float32)) \
            / np.asarray(IMAGENET_STD, np.float32)
        arr = a.transpose(0, 3, 1, 2)
    x = torch.from_numpy(np.require(arr, np.float32, ["C", "W"]))  # NCHW-contiguous (CPU convs), writable
    if x.dim() == 3:
        x = x[None]
    return x


def softmax_np(x):
    x = np.asarray(x, np.float32)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def topk_np(p, k: int):
    """[(indices, values)] per row, highest first."""
    idx = np.argpartition(-p, k - 1, axis=-1)[:, :k]
    vals = np.take_along_axis(p, idx, -1)
    order = np.argsort(-vals, axis=-1)
    return np.take_along_axis(idx, order, -1), np.take_along_axis(vals, order, -1)


def _predict_text(s, body):
    """BERT-style sequence classification: {"model", "input_ids", "token_type_ids"?,
    "attention_mask"?} -> class probabilities."""
    model = body.get("model") or "bert-base"
    ids = np.asarray(body["input_ids"], dtype=np.int64)
    if ids.ndim == 1:
        ids = ids[None]
    tt = body.get("token_type_ids")
    am = body.get("attention_mask")
    tt = np.asarray(tt, dtype=np.int64).reshape(ids.shape) if tt is not None else None
    am = np.asarray(am, dtype=np.int64).reshape(ids.shape) if am is not None else None
    with phase("load"):
        backend = s.text(model)
    t0 = time.perf_counter()
    with phase("infer"):
        if hasattr(backend, "infer_np"):  # plan-backed: torch-free
            logits = backend.infer_np(ids, tt, am)
        else:
            import torch
            def tens(a):
                return None if a is None else torch.from_numpy(a)
            logits = backend(tens(ids), tens(tt), tens(am)).float().numpy()
    dt = (time.perf_counter() - t0) * 1e3
    probs = softmax_np(logits)
    return _json({"model": model, "backend": backend.backend, "batch": int(ids.shape[0]),
                  "probs": [[round(float(p), 6) for p in row] for row in probs],
                  "label": [int(i) for i in probs.argmax(-1)], "timing_ms": round(dt, 3)})


@app.route("/predict", methods=["POST"])
def predict():
    s = get_server()
    if request.mimetype != "application/octet-stream":
        body = request.get_json(force=True, silent=True) or {}
        if "input_ids" in body:
            return _predict_text(s, body)
    with phase("decode"):
        model, arr = decode_input(request)
    with phase("load"):
        backend = s.vision(model)
    t0 = time.perf_counter()
    dp = _DP["member"]
    if (dp is not None and dp.alive and model == _DP["model"] and arr.dtype == np.uint8 and arr.shape[0] > 1
            and tuple(arr.shape[1:]) == _DP["item_shape"]):
        with phase("dp_scatter_gather"):  # C2 scatter -> every GPU's shard -> C3 gather
            out = dp.submit(arr)
        logits, probs = out, softmax_np(out)
    elif arr.dtype == np.uint8 and hasattr(backend, "infer_u8") and backend.accepts_u8(arr.shape):
        with phase("infer"):  # torch-free: pinned input -> captured graph (preprocess on device)
            out = backend.infer_u8(arr)
        logits = None if backend.probs else out
        probs = out if backend.probs else softmax_np(out)
    else:
        prz = getattr(backend, "resize", None)  # a resize plan refused the image: above its maximum
        if prz is not None and arr.dtype == np.uint8 and arr.ndim == 4:
            check_image_size(arr, (prz["resize"], prz["crop"], prz["max_h"], prz["max_w"]))
        with phase("preprocess"):
            x = to_model_input(arr, s.resize_spec(model))
        with phase("infer"):
            lg = backend(x)
        logits = lg.float().numpy()
        probs = softmax_np(logits)
    dt = (time.perf_counter() - t0) * 1e3
    k = min(5, probs.shape[-1])
    ti, tp = topk_np(probs, k)
    out = {"model": model, "backend": backend.backend, "batch": int(arr.shape[0]),
           "top5": [[[int(i), round(float(p), 6)] for i, p in zip(r_i, r_p)] for r_i, r_p in zip(ti, tp)],
           "timing_ms": round(dt, 3)}
    if request.args.get("logits") and logits is not None:
        out["logits"] = logits.tolist()
    return _json(out)


def _text_arrays(body):
    ids = np.asarray(body["input_ids"], dtype=np.int64)
    if ids.ndim == 1:
        ids = ids[None]
    tt = body.get("token_type_ids")
    am = body.get("attention_mask")
    tt = np.asarray(tt, dtype=np.int64).reshape(ids.shape) if tt is not None else None
    am = np.asarray(am, dtype=np.int64).reshape(ids.shape) if am is not None else None
    return ids, tt, am


def _need_embed(backend, model):
    if getattr(backend, "embed", None) is None:
        raise ValueError(f"{model} is served without extra.embed (a classification model): POST /predict, or set "
                         f'"embed": {{"pooling": "mean", "normalize": true}} in its settings block')
    return backend.embed


def _embed_vectors(s, limit: bool = False):
    """The request's inputs embedded by the model's backend -> (model, backend, embed spec, vectors, n, t0).
    ``limit``: refuse more inputs than the backend's batch (POST /search: one replay per request)."""
    body = {}
    if request.mimetype != "application/octet-stream" and request.mimetype not in IMAGE_TYPES:
        body = request.get_json(force=True, silent=True) or {}
    if "input_ids" in body:
        model = body.get("model") or "bert-base"
        ids, tt, am = _text_arrays(body)
        with phase("load"):
            backend = s.text(model)
        e = _need_embed(backend, model)
        _check_inputs(limit, int(ids.shape[0]), backend)
        t0 = time.perf_counter()
        with phase("infer"):
            if hasattr(backend, "embed_np"):  # plan-backed: torch-free
                vec = backend.embed_np(ids, tt, am)
            else:
                import torch
                def tens(a):
                    return None if a is None else torch.from_numpy(a)
                vec = backend.embed_ids(tens(ids), tens(tt), tens(am)).float().numpy()
        n = int(ids.shape[0])
    else:
        with phase("decode"):
            model, arr = decode_input(request)
        with phase("load"):
            backend = s.vision(model)
        e = _need_embed(backend, model)
        _check_inputs(limit, int(arr.shape[0]), backend)
        t0 = time.perf_counter()
        if arr.dtype == np.uint8 and hasattr(backend, "embed_u8") and backend.accepts_u8(arr.shape):
            with phase("infer"):
                vec = backend.embed_u8(arr)
        else:
            prz = getattr(backend, "resize", None)  # a resize plan refused the image: above its maximum
            if prz is not None and arr.dtype == np.uint8 and arr.ndim == 4:
                check_image_size(arr, (prz["resize"], prz["crop"], prz["max_h"], prz["max_w"]))
            with phase("preprocess"):
                x = to_model_input(arr, s.resize_spec(model))
            with phase("infer"):
                vec = backend.embed_x(x).float().numpy()
        n = int(arr.shape[0])
    return model, backend, e, vec, n, t0


def _check_inputs(limit: bool, n: int, backend) -> None:
    if limit and n > int(getattr(backend, "batch", 1)):
        raise ValueError(f"{n} inputs exceed the batch of {backend.batch} this model is served with")


@app.route("/embed", methods=["POST"])
def embed():
    """One pooled vector per sequence (``input_ids`` [+ ``attention_mask``, ``token_type_ids``]) or
    per image (the bodies of /predict) from a model whose settings block has ``extra.embed``."""
    model, backend, e, vec, n, t0 = _embed_vectors(get_server())
    dt = (time.perf_counter() - t0) * 1e3
    vec = np.ascontiguousarray(vec, np.float32)
    if "application/octet-stream" in request.headers.get("Accept", ""):
        buf = io.BytesIO()
        np.save(buf, vec, allow_pickle=False)
        return Response(response=buf.getvalue(), status=200, mimetype="application/octet-stream")
    return _json({"model": model, "backend": backend.backend, "batch": n, "dim": int(vec.shape[1]),
                  "pooling": e["pooling"], "normalized": bool(e["normalize"]),
                  "embeddings": [[float(v) for v in row] for row in vec], "timing_ms": round(dt, 3)})


def _embedding_backend(s, model):
    """The backend of an embedding model named in a ``vectors`` request (text or vision)."""
    name = s.spec(model).name
    with phase("load"):
        backend = s.vision(model) if name.startswith(("vit", "resnet")) else s.text(model)
    return backend


def _u32_field(value, name: str) -> int:
    if not isinstance(value, int) or isinstance(value, bool) or not 0 <= value <= 0xFFFFFFFF:
        raise ValueError(f"{name} must be an integer in 0..4294967295, got {value!r}")
    return value


def _search_filter(body):
    """``"filter": {"mask": m, "value": v}`` or the shorthand ``"tag": t`` (mask 0xffffffff) -> (mask, value)."""
    if "filter" in body:
        f = body["filter"]
        if not isinstance(f, dict) or set(f) != {"mask", "value"}:
            raise ValueError('filter must be {"mask": m, "value": v}')
        if "tag" in body:
            raise ValueError("give one of filter and tag")
        return _u32_field(f["mask"], "filter.mask"), _u32_field(f["value"], "filter.value")
    if "tag" in body:
        return 0xFFFFFFFF, _u32_field(body["tag"], "tag")
    return None


def _writable_index(s, body):
    """The model's index for a mutation route: 400 without ``extra.index``, 403 without
    ``extra.index_writable: true``."""
    model = body.get("model") or request.args.get("model") or "bert-base"
    extra = s.spec(model).extra
    if not extra.get("index"):
        raise ValueError(f'{model} is served without extra.index: set "index": "<path or artifact key>" in its '
                         f"settings block (hipzap index writes one)")
    if extra.get("index_writable") is not True:
        return model, None
    return model, s.index(model, _embedding_backend(s, model))


def _forbidden(model):
    return _json({"error": "Forbidden", "message": f'{model}: the index is read-only; set "index_writable": true in its settings block'}, 403)


@app.route("/index/add", methods=["POST"])
def index_add():
    """Append rows to the model's index: the vectors /embed gives for the body, or ``{"model", "vectors"}``;
    optional ``"tags"`` (integers 0..2^32-1) and ``"labels"`` (required iff the index has labels)."""
    s = get_server()
    body = {}
    if request.mimetype != "application/octet-stream" and request.mimetype not in IMAGE_TYPES:
        body = request.get_json(force=True, silent=True) or {}
    model, index = _writable_index(s, body)
    if index is None:
        return _forbidden(model)
    if "vectors" in body:
        try:
            vec = np.asarray(body["vectors"], dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("vectors must be a list of equally long lists of numbers") from None
        vec = vec[None] if vec.ndim == 1 else vec
    else:
        vec = np.ascontiguousarray(_embed_vectors(s)[3], np.float32)
    tags = body.get("tags")
    if tags is not None:
        if not isinstance(tags, list):
            raise ValueError("tags must be a list of integers in 0..4294967295")
        tags = np.asarray([_u32_field(t, "tags") for t in tags], np.uint32)
    labels = body.get("labels")
    if labels is not None and (not isinstance(labels, list) or not all(isinstance(x, str) for x in labels)):
        raise ValueError("labels must be a list of strings")
    ids = index.add(vec, tags=tags, labels=labels)
    return _json({"model": model, "ids": [int(i) for i in ids], "count": int(index.count)})


@app.route("/index/delete", methods=["POST"])
def index_delete():
    s = get_server()
    body = request.get_json(force=True, silent=True) or {}
    model, index = _writable_index(s, body)
    if index is None:
        return _forbidden(model)
    ids = body.get("ids")
    if not isinstance(ids, list) or not all(isinstance(i, int) and not isinstance(i, bool) for i in ids):
        raise ValueError("ids must be a list of integers")
    return _json({"model": model, "deleted": index.delete(ids)})


@app.route("/index/save", methods=["POST"])
def index_save():
    """Write the index, ids and tombstones kept, to the path it was opened from."""
    s = get_server()
    body = request.get_json(force=True, silent=True) or {}
    model, index = _writable_index(s, body)
    if index is None:
        return _forbidden(model)
    hdr = index.save()
    return _json({"model": model, "path": index.path, "count": int(hdr["count"])})


@app.route("/search", methods=["POST"])
def search():
    """The ``k`` nearest rows of the model's vector index (``extra.index``) per query. The queries are the
    vectors /embed gives for the same body, or ``{"model", "vectors": [[...]]}``; a cosine index gets them
    L2-normalised in fp32. ``"k"`` (JSON field or query argument): 1..128, default 10. ``"filter": {"mask",
    "value"}`` or ``"tag": t`` restricts the answer to the rows whose tag passes ``(tag & mask) == value``.
    ``"refine"`` (an index with rescore rows): the candidates the fp8 scan hands the exact bf16 second stage,
    an integer in k..128, ``0`` for none; absent or null: 128 on such an index. The answer's ``"refine"`` is the
    R used, 0 if none. ``"nprobe"`` (an IVF index): the lists each query scans, an integer in 1..min(nlist, 128)
    or ``"all"``; absent: ``extra.index_nprobe``, else the file's default. The answer of an IVF index carries
    ``"ivf": true`` and the ``"nprobe"`` used (``"all"`` when every list was scanned). ``"nprobe"`` and ``"refine"``
    go together on an fp8 IVF index with rescore rows (a version-7 file): the probed lists give the R candidates.
    ``"batch": true`` answers through ``search_batch`` (every query in one pass of the MFMA scan, exact
    rescoring, the unproven queries re-run through ``search``): the same results, plus ``"certain"`` (one boolean per
    query, all true here) in the JSON answer. 400 on an index kind ``search_batch`` refuses, and with a filter,
    ``refine`` or ``nprobe``, which the batch path does not take."""
    from ..search import MAX_K, check_k, check_queries, normalize_rows
    s = get_server()
    body = {}
    if request.mimetype != "application/octet-stream" and request.mimetype not in IMAGE_TYPES:
        body = request.get_json(force=True, silent=True) or {}
    k = body.get("k", request.args.get("k", 10))
    if isinstance(k, str) and k.lstrip("-").isdigit():
        k = int(k)
    k = check_k(k)
    if "vectors" in body:
        model = body.get("model") or request.args.get("model") or "bert-base"
        backend = _embedding_backend(s, model)
        e = _need_embed(backend, model)
        index = s.index(model, backend)
        t0 = time.perf_counter()
        try:
            q = np.asarray(body["vectors"], dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("vectors must be a list of equally long lists of numbers") from None
        q = check_queries(q, index.dim)
    else:
        model, backend, e, vec, _, t0 = _embed_vectors(s, limit=True)
        index = s.index(model, backend)
        q = check_queries(vec, index.dim)
    if index.metric == "cosine":
        q = normalize_rows(q)
    filt = _search_filter(body)
    batch = body.get("batch", False)
    if not isinstance(batch, bool):
        raise ValueError(f"batch must be true or false, got {batch!r}")
    nprobe = body.get("nprobe")
    if batch:
        index._check_batch(k, None)  # ValueError -> 400: an index kind the batch path refuses
        if filt is not None or nprobe is not None or body.get("refine") is not None:
            raise ValueError("batch takes no filter, tag, refine or nprobe")
    if index.ivf is not None and nprobe is not None and nprobe != "all" and (
            isinstance(nprobe, bool) or not isinstance(nprobe, int) or not 1 <= nprobe <= min(index.ivf["nlist"], MAX_K)):
        raise ValueError(f"nprobe must be an integer in 1..{min(index.ivf['nlist'], MAX_K)} or \"all\", got {nprobe!r}")
    lists = index._nprobe(nprobe, body.get("refine"))  # ValueError -> 400 (nprobe without lists, refine with them)
    refine = index._refine(body.get("refine"), k)  # ValueError -> 400
    certain = None
    with phase("search"):
        if batch:
            scores, ids, certain = index.search_batch(q, k, fallback=True)
        else:
            scores, ids = index.search(q, k, filter=filt, refine=refine, nprobe=nprobe)
    dt = (time.perf_counter() - t0) * 1e3
    if "application/octet-stream" in request.headers.get("Accept", ""):
        out = np.empty(ids.shape, dtype=[("id", "<i4"), ("score", "<f4")])
        out["id"], out["score"] = ids, scores
        buf = io.BytesIO()
        np.save(buf, out, allow_pickle=False)
        return Response(response=buf.getvalue(), status=200, mimetype="application/octet-stream")
    labels = index.labels

    def hit(i, sc):
        h = {"id": int(i), "score": float(sc) if np.isfinite(sc) else None}
        if labels is not None and i >= 0:
            h["label"] = labels[i]
        return h
    return _json({"model": model, "backend": backend.backend, "metric": index.metric, "dtype": index.dtype, "refine": refine, "k": k,
                  "count": int(index.count), **({"ivf": True, "nprobe": lists or "all"} if index.ivf is not None else {}),
                  **({"batch": True, "certain": [bool(c) for c in certain]} if batch else {}),
                  "results": [[hit(i, sc) for i, sc in zip(ri, rs)] for ri, rs in zip(ids, scores)],
                  "timing_ms": round(dt, 3)})


@app.route("/index/neighbors", methods=["POST"])
def index_neighbors():
    """The ``k`` nearest live rows of stored rows of the model's index (``extra.index``; it only reads, so no
    ``extra.index_writable``): ``{"model", "ids": [...], "k"?: 10, "include_self"?: false}``. A row is left out of its
    own list unless ``include_self``. The answer has /search's two shapes: JSON hits (with labels where the index
    has them) or, with ``Accept: application/octet-stream``, a structured ``.npy`` [n, k] (id, score). 400 with the
    index's message for an id outside [0, count), a deleted id, k outside 1..128, and an fp8 or IVF index or a
    ``dim % 32 != 0`` one, for which neighbours are not built."""
    from ..search import check_k
    s = get_server()
    body = request.get_json(force=True, silent=True) or {}
    model = body.get("model") or request.args.get("model") or "bert-base"
    k = body.get("k", request.args.get("k", 10))
    if isinstance(k, str) and k.lstrip("-").isdigit():
        k = int(k)
    k = check_k(k)
    ids = body.get("ids")
    if not isinstance(ids, list) or not ids or not all(isinstance(i, int) and not isinstance(i, bool) for i in ids):
        raise ValueError("ids must be a non-empty list of integers")
    include_self = body.get("include_self", False)
    if not isinstance(include_self, bool):
        raise ValueError(f"include_self must be true or false, got {include_self!r}")
    if not s.spec(model).extra.get("index"):
        raise ValueError(f'{model} is served without extra.index: set "index": "<path or artifact key>" in its '
                         f"settings block (hipzap index writes one)")
    backend = _embedding_backend(s, model)
    index = s.index(model, backend)
    t0 = time.perf_counter()
    with phase("search"):
        scores, near = index.neighbors(ids, k, include_self=include_self)  # ValueError -> 400
    dt = (time.perf_counter() - t0) * 1e3
    if "application/octet-stream" in request.headers.get("Accept", ""):
        out = np.empty(near.shape, dtype=[("id", "<i4"), ("score", "<f4")])
        out["id"], out["score"] = near, scores
        buf = io.BytesIO()
        np.save(buf, out, allow_pickle=False)
        return Response(response=buf.getvalue(), status=200, mimetype="application/octet-stream")
    labels = index.labels

    def hit(i, sc):
        h = {"id": int(i), "score": float(sc) if np.isfinite(sc) else None}
        if labels is not None and i >= 0:
            h["label"] = labels[i]
        return h
    return _json({"model": model, "backend": backend.backend, "metric": index.metric, "dtype": index.dtype, "k": k,
                  "include_self": include_self, "count": int(index.count), "ids": ids,
                  "results": [[hit(i, sc) for i, sc in zip(ri, rs)] for ri, rs in zip(near, scores)],
                  "timing_ms": round(dt, 3)})


@app.route("/health", methods=["GET"])
def health():
    s = get_server()
    info = {"status": "ok", "backend": s.backend, "models": s.loaded()}
    if CLUSTER:
        m, c = CLUSTER.get("member"), CLUSTER.get("coordinator")
        info["cluster"] = {"rank": CLUSTER["rank"], "world": CLUSTER["world"], "device": CLUSTER["device"],
                           "cold_start_ms": CLUSTER["cold_start_ms"],
                           "members": m.members if m else None, "epoch": m.epoch if m else None,
                           "health": m.health if m else None, "dp": _DP["member"] is not None,
                           "reforms": c.reforms if c else (m.reforms if m else None)}
    if s.backend == "gpu":
        info["devices"] = list(s.settings.devices)
        if "torch" in sys.modules:  # names only when torch is loaded anyway (never imported for this)
            import torch
            info["device_names"] = [torch.cuda.get_device_name(d) for d in s.settings.devices]
    return _json(info)


@app.route("/metrics", methods=["GET"])
def metrics():
    from ..utils.gpu_metrics import render as gpu_render
    return Response(METRICS.render() + gpu_render(), mimetype="text/plain; version=0.0.4")
