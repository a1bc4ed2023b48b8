"""hipzap command line: serve | pack | tune | upload | info | bench.

    python -m hipzap serve --port 8082            # local dev server (reference: main.py:115-127)
    python -m hipzap pack --model resnet50 --ckpt m.pth --out m.hzpack
    python -m hipzap plan --model resnet50 --ckpt m.pth [--contexts 24]  # torch-free cold-start image
    python -m hipzap plan --model resnet50 --ckpt m.pth --resize 256 [--max-image 1024x1024]  # any-size images
    python -m hipzap plan --model bert-base --ckpt bert.pth --embed [--pooling mean|cls] [--no-normalize]  # vectors
    python -m hipzap tune --model resnet50 --batch 1 --concurrent 1 8
    python -m hipzap upload --models-dir ./models  # scripts/upload_models.py parity
    python -m hipzap index --vectors v.npy [--labels labels.json] [--metric cosine|ip] --out x.hzidx  # vector index
    python -m hipzap index --embed-plan bert.pth.emb.hzplan --ids ids.npy [--mask mask.npy] --out x.hzidx
    python -m hipzap plan --model resnet50 --ckpt m.pth --embed [--resize 256] [--no-normalize]  # image vectors
    python -m hipzap index --embed-plan m.pth.emb.hzplan --images imgs.npy --out x.hzidx  # uint8 [N, H, W, 3]
    python -m hipzap index --from-index a.hzidx --dtype fp8 --out b.hzidx  # requantise a bf16 index (ids kept)
    python -m hipzap index --vectors v.npy --dtype fp8 --rescore --out c.hzidx  # fp8 scan + bf16 rescoring (version 4)
    python -m hipzap index --vectors v.npy --dtype bin --rescore --out d.hzidx  # sign-bit scan + bf16 rescoring (version 9)
    python -m hipzap index --vectors v.npy --dtype pq --pq-m 96 --rescore --out e.hzidx  # product quantisation (version 11)
    python -m hipzap index --vectors v.npy --dtype pq --pq-m 96 --pq-backend gpu --out f.hzidx  # trained and encoded on the GPU
    python -m hipzap info [x.hzidx]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys


def cmd_serve(a):
    from .serve.settings import load_settings
    st = load_settings(a.settings, a.stage)
    host, port = a.host or st.host, a.port or st.port
    if a.gpus and a.gpus > 1:  # one worker process per GPU sharing the listening socket (serve/cluster.py)
        from .serve.cluster import launch
        sys.exit(launch(a.gpus, host, port, settings=a.settings, stage=a.stage))
    from .serve.app import app, serve_threaded, set_server
    from .serve.server import ModelServer, PlanVisionBackend
    srv = ModelServer(st)  # the settings named on the command line, not the default file
    set_server(srv)
    if srv.backend == "gpu" and os.environ.get("HIPZAP_NATIVE_HTTP", "1") != "0":
        # native HTTP/1.1 front end: POST /predict for the plan-backed default model in C++,
        # everything else through the Flask app (serve/native_http.py)
        from .serve.native_http import NativeHTTPServer, listening_socket
        be = srv.vision(st.default_model)  # cold start before the port opens
        # (a resize plan's requests are encoded images of any size: they take the Flask route)
        fast = be if isinstance(be, PlanVisionBackend) and be.resize is None else None
        if os.environ.get("HIPZAP_LM_PRELOAD", "0") == "1":
            srv.lm()  # GET /inference backend before the port opens (else on its first request)
        http = NativeHTTPServer(app, listening_socket(host, port), fast=fast, server=srv)
        print(f"hipzap serving stage {st.stage} on {host}:{port} (native http, fast route: "
              f"{fast.name if fast else None}, native GET /inference: {http.lm_native})", flush=True)
        http.serve_forever()
        return
    from werkzeug.serving import WSGIRequestHandler
    WSGIRequestHandler.protocol_version = "HTTP/1.1"  # keep-alive: no TCP handshake per request
    print(f"hipzap serving stage {st.stage} on {host}:{port} (models bucket {st.models_bucket!r})", flush=True)
    app.run(host=host, port=port, debug=False, threaded=serve_threaded())


def cmd_pack(a):
    import hashlib

    import torch

    from .engine.packfile import save_packed
    from .models import registry
    ad = registry.get(a.model)
    sd = torch.load(a.ckpt, map_location="cpu", weights_only=True)
    params, cfg = ad.pack(sd, "cpu")
    h = hashlib.sha256(open(a.ckpt, "rb").read()).hexdigest()
    save_packed(params, cfg, a.out, h)
    print(json.dumps({"out": a.out, "entries": len(params), "source_sha256": h}))


def cmd_plan(a):
    from .engine.plan import export_from_checkpoint
    from .imgeom import resize_spec
    from .lite import read_meta
    from .models import registry
    crop = a.crop or getattr(registry.get(a.model), "image", 224)
    embed = {"pooling": a.pooling or ("cls" if a.model.startswith("vit") else "mean"),
             "normalize": not a.no_normalize} if a.embed else None
    if embed is None and (a.pooling or a.no_normalize):
        raise SystemExit("--pooling / --no-normalize go with --embed")
    if embed is not None and a.model.startswith("resnet") and embed["pooling"] != "mean":
        raise SystemExit(f"plan: --pooling {embed['pooling']} does not apply to {a.model}: a ResNet embedding is its "
                         f"global average pool (--pooling mean, the default)")
    out = export_from_checkpoint(a.model, a.ckpt, a.out, batch=a.batch, contexts=a.contexts, probs=a.probs,
                                 dp_shard=a.dp_shard, seq_len=a.seq_len,
                                 resize=resize_spec(a.resize, crop, a.max_image), embed=embed)
    m = read_meta(out)
    print(json.dumps({"out": out, "ops": m["n_ops"], "blob_bytes": m["blob_bytes"], "source": m["source"],
                      **({"resize": m["resize"]} if m.get("resize") else {}),
                      **({"embed": m["embed"]} if m.get("embed") else {})}))


def cmd_tune(a):
    sys.argv = ["tune", "--model", a.model, "--batch", *map(str, a.batch), "--concurrent", *map(str, a.concurrent)]
    from .engine import tune
    tune.main()


def cmd_upload(a):
    from .serve.artifacts import ArtifactStore
    from .serve.settings import load_settings
    st = load_settings(a.settings, a.stage)
    bucket = a.bucket or st.models_bucket
    if not bucket:
        sys.exit("no models bucket: set aws_environment_variables.models_bucket in zappa_settings.json or --bucket")
    copied = ArtifactStore(bucket).upload_dir(a.models_dir)
    print(json.dumps({"bucket": bucket, "copied": copied}))


def cmd_index(a):
    """Write a .hzidx vector index (hipzap/search.py) from ready vectors, or from the vectors an embedding
    plan gives for rows of token ids (on the GPU, torch-free)."""
    import numpy as np

    from .search import convert_index, write_index
    if a.ivf is not None and a.dtype == "bin":
        raise SystemExit("index: --ivf with --dtype bin: IVF lists over binary rows are not built")
    if a.ivf is not None and a.dtype == "pq":
        raise SystemExit("index: --ivf with --dtype pq: IVF lists over pq8 rows are not built")
    if a.dtype == "pq" and a.pq_m is None:
        raise SystemExit("index: --dtype pq needs --pq-m M, the code bytes per row (a multiple of 16 in 16..96 that divides dim)")
    if a.dtype != "pq" and (a.pq_m is not None or a.pq_iters is not None or a.pq_seed is not None):
        raise SystemExit("index: --pq-m, --pq-iters and --pq-seed go with --dtype pq")
    if a.dtype != "pq" and a.pq_backend is not None:
        raise SystemExit("index: --pq-backend goes with --dtype pq")
    pq = {} if a.dtype != "pq" else {"pq_m": a.pq_m, "pq_iters": 10 if a.pq_iters is None else a.pq_iters,
                                     "pq_seed": a.pq_seed or 0, "pq_backend": a.pq_backend or "cpu"}
    if a.rescore and a.dtype not in ("fp8", "bin", "pq"):
        raise SystemExit(f"index: --rescore goes with --dtype fp8: a {a.dtype} index already holds its rows in bf16, "
                         f"there is nothing to re-score against")
    if a.from_index is not None:
        if a.vectors is not None or a.embed_plan is not None or a.labels or a.tags or a.ids or a.mask or a.images:
            raise SystemExit("index: --from-index takes only --dtype, --rescore, --ivf with --nprobe / --ivf-seed, and --out")
        if a.ivf is None and (a.nprobe is not None or a.ivf_seed is not None):
            raise SystemExit("index: --nprobe and --ivf-seed go with --ivf NLIST")
        if a.ivf is None and a.ivf_backend != "cpu":
            raise SystemExit("index: --ivf-backend goes with --ivf NLIST")
        try:
            hdr = convert_index(a.from_index, a.out, a.dtype, rescore=a.rescore, ivf=a.ivf, nprobe=a.nprobe,
                                ivf_seed=a.ivf_seed or 0, ivf_backend=a.ivf_backend, device=a.device, **pq)
        except ValueError as e:
            raise SystemExit(f"index: {e}") from None
        print(json.dumps({"out": a.out, **{k: v for k, v in hdr.items() if k != "labels"}, "labels": "labels" in hdr}))
        return
    if (a.vectors is None) == (a.embed_plan is None):
        raise SystemExit("index: give one of --vectors, --embed-plan and --from-index")
    embed, model = None, a.model
    if a.images and (a.ids or a.mask):
        raise SystemExit("index: --images (a vision embedding plan) does not combine with --ids / --mask (a text one)")
    if a.vectors is not None:
        if a.ids or a.mask or a.images:
            raise SystemExit("index: --ids / --mask / --images go with --embed-plan")
        vec = np.load(a.vectors, allow_pickle=False)
    elif a.images:
        vec, embed, pm = _embed_images(a)
        model = model or pm
    else:
        if not a.ids:
            raise SystemExit("index: --embed-plan needs --ids (an .npy of token-id rows)")
        from .serve.server import PlanTextBackend
        from .serve.settings import ModelSpec
        ids = np.load(a.ids, allow_pickle=False)
        mask = np.load(a.mask, allow_pickle=False) if a.mask else None
        be = PlanTextBackend(a.model or "bert-base", a.embed_plan, a.device, ModelSpec(name=a.model or "bert-base"))
        if be.embed is None:
            raise SystemExit(f"index: {a.embed_plan} is not an embedding plan (hipzap plan --embed)")
        vec, embed = be.embed_np(ids, None, mask), dict(be.embed)
        model = model or be.meta.get("model")
    labels = json.load(open(a.labels)) if a.labels else None
    tags = np.load(a.tags, allow_pickle=False) if a.tags else None
    if a.ivf is None and (a.nprobe is not None or a.ivf_seed is not None):
        raise SystemExit("index: --nprobe and --ivf-seed go with --ivf NLIST")
    if a.ivf is None and a.ivf_backend != "cpu":
        raise SystemExit("index: --ivf-backend goes with --ivf NLIST")
    if a.ivf is not None and a.dtype == "fp8":  # the lists are trained on the bf16 rows, which are then quantised
        tmp = a.out + ".bf16-ivf.tmp"
        try:
            write_index(tmp, vec, a.metric, labels=labels, model=model or "", embed=embed, tags=tags, ivf=a.ivf,
                        nprobe=a.nprobe, ivf_seed=a.ivf_seed or 0, ivf_backend=a.ivf_backend, device=a.device)
            hdr = convert_index(tmp, a.out, "fp8", rescore=a.rescore)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    else:
        try:
            hdr = write_index(a.out, vec, a.metric, labels=labels, model=model or "", embed=embed, tags=tags, dtype=a.dtype,
                              rescore=a.rescore, ivf=a.ivf, nprobe=a.nprobe, ivf_seed=a.ivf_seed or 0,
                              ivf_backend=a.ivf_backend, device=a.device, **pq)
        except ValueError as e:
            if a.dtype != "pq":
                raise
            raise SystemExit(f"index: {e}") from None
    print(json.dumps({"out": a.out, **{k: v for k, v in hdr.items() if k != "labels"}, "labels": labels is not None}))


def _embed_images(a):
    """``hipzap index --embed-plan P --images imgs.npy``: the vectors a vision embedding plan (ResNet or ViT)
    gives for uint8 [N, H, W, 3] images, on the GPU, torch-free -> (vectors, embed spec, the plan's model)."""
    import numpy as np

    from .lite import read_meta
    from .serve.server import PlanVisionBackend
    from .serve.settings import ModelSpec
    meta = read_meta(a.embed_plan)
    if meta.get("kind") == "text":
        raise SystemExit(f"index: {a.embed_plan} is a text plan: its rows come from --ids, not --images")
    if not meta.get("embed"):
        raise SystemExit(f"index: {a.embed_plan} is not an embedding plan (hipzap plan --embed)")
    imgs = np.load(a.images, allow_pickle=False)
    name = a.model or meta.get("model") or "resnet50"
    be = PlanVisionBackend(name, a.embed_plan, a.device, ModelSpec(name=name))
    if imgs.dtype != np.uint8 or not be.accepts_u8(imgs.shape):
        want = f"at most {be.resize['max_h']} x {be.resize['max_w']}" if be.resize else f"{list(be.in_shape[1:])}"
        raise SystemExit(f"index: --images is a uint8 array [N, H, W, 3] with images {want} for this plan, got "
                         f"{imgs.dtype} {list(imgs.shape)}")
    return be.embed_u8(imgs), dict(be.embed), meta.get("model")


def cmd_info(a):
    if a.path:  # a .hzidx file: its header
        from .search import file_info, read_header
        print(json.dumps({"path": a.path, **read_header(a.path), **file_info(a.path)}, indent=1))
        return
    import torch

    from . import __version__, _native
    from .models import registry
    info = {"version": __version__, "models": registry.names(), "native_library": str(_native._LIB_PATH),
            "native_built": _native.available(), "gpu": torch.cuda.is_available()}
    if torch.cuda.is_available():
        info["devices"] = [torch.cuda.get_device_name(i) for i in range(torch.cuda.device_count())]
    print(json.dumps(info, indent=1))


def cmd_knn(a):
    """The kNN graph of a plain bf16 index -> an .npz with ``ids`` int32 [count, k] and ``scores`` float32 [count, k]
    (-1 / -inf in a deleted row's lists)."""
    import numpy as np

    from .search import open_index
    try:
        with open_index(a.index, a.backend, a.device) as ix:
            ids, scores = ix.knn_graph(a.k, block=a.block) if a.block else ix.knn_graph(a.k)
    except ValueError as e:
        sys.exit(f"hipzap knn: {e}")
    with open(a.out, "wb") as f:
        np.savez(f, ids=ids, scores=scores)
    print(json.dumps({"index": a.index, "out": a.out, "count": int(ids.shape[0]), "k": a.k, "backend": a.backend,
                      "rows_with_neighbors": int((ids[:, 0] >= 0).sum())}))


def cmd_cluster(a):
    """k-means over the live rows of a plain bf16 index -> an .npz with ``centroids`` uint16 [k, dim] (bf16 bits),
    ``assign`` int32 [count] and ``score`` float32 [count] (-1 / -inf for a deleted row)."""
    import numpy as np

    from .search import open_index
    try:
        with open_index(a.index, a.backend, a.device) as ix:
            cent, assign, score = ix.cluster(a.k, iters=a.iters, seed=a.seed)
    except ValueError as e:
        sys.exit(f"hipzap cluster: {e}")
    with open(a.out, "wb") as f:
        np.savez(f, centroids=cent, assign=assign, score=score)
    sizes = np.bincount(assign[assign >= 0], minlength=a.k)
    print(json.dumps({"index": a.index, "out": a.out, "count": int(assign.size), "k": a.k, "iters": a.iters, "seed": a.seed,
                      "backend": a.backend, "clustered_rows": int((assign >= 0).sum()), "empty_clusters": int((sizes == 0).sum()),
                      "largest_cluster": int(sizes.max())}))


def cmd_bench(a, rest):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.exit(subprocess.call([sys.executable, os.path.join(root, "bench.py"), *rest]))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="hipzap")
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("serve")
    s.add_argument("--host", default=None)
    s.add_argument("--port", type=int, default=None)
    s.add_argument("--stage", default=None)
    s.add_argument("--settings", default=None)
    s.add_argument("--gpus", type=int, default=0, help="> 1: data-parallel cluster, one worker process per GPU")
    p = sub.add_parser("pack")
    p.add_argument("--model", required=True)
    p.add_argument("--ckpt", required=True)
    p.add_argument("--out", required=True)
    pl = sub.add_parser("plan")
    pl.add_argument("--model", required=True)
    pl.add_argument("--ckpt", required=True)
    pl.add_argument("--out", default=None, help="default: <ckpt>.hzplan")
    pl.add_argument("--batch", type=int, default=1)
    pl.add_argument("--contexts", type=int, default=1, help="request concurrency the launch configs are tuned for")
    pl.add_argument("--probs", action="store_true", help="softmax head on device")
    pl.add_argument("--seq-len", type=int, default=None,
                    help="text models: captured sequence length (default 128, at most the checkpoint's positions)")
    pl.add_argument("--dp-shard", type=int, default=None,
                    help="also write <ckpt>.dp<S>.hzplan: the per-GPU shard program of batched DP requests")
    pl.add_argument("--resize", type=int, default=None,
                    help="ResNet / ViT: write a RESIZE plan (with --embed: <ckpt>.emb.rz.hzplan) -- requests are uint8 images of any size, the shorter "
                         "side resized to this (antialiased bilinear), centre-cropped and normalised on the GPU")
    pl.add_argument("--embed", action="store_true",
                    help="BERT / ViT / ResNet: write an EMBEDDING plan (<ckpt>.emb.hzplan) -- the output is one pooled vector "
                         "per sequence / image (POST /embed) instead of class logits")
    pl.add_argument("--pooling", choices=["mean", "cls"], default=None,
                    help="with --embed: masked token mean or the CLS token (default: mean for BERT, cls for ViT; "
                         "a ResNet pools by the mean only)")
    pl.add_argument("--no-normalize", action="store_true", help="with --embed: do not L2-normalise the vectors")
    pl.add_argument("--crop", type=int, default=None, help="with --resize: crop size (default: the model's image size)")
    pl.add_argument("--max-image", default=None,
                    help="with --resize: largest request image, HEIGHTxWIDTH (default 1024x1024)")
    t = sub.add_parser("tune")
    t.add_argument("--model", default="resnet50")
    t.add_argument("--batch", type=int, nargs="+", default=[1])
    t.add_argument("--concurrent", type=int, nargs="+", default=[1])
    u = sub.add_parser("upload")
    u.add_argument("--models-dir", default="./models")
    u.add_argument("--bucket", default=None)
    u.add_argument("--stage", default=None)
    u.add_argument("--settings", default=None)
    ix = sub.add_parser("index")
    ix.add_argument("--vectors", default=None, help="an .npy float array [N, D]")
    ix.add_argument("--embed-plan", default=None,
                    help="an embedding plan: the vectors of the --ids rows (text) or of the --images (vision), on the GPU")
    ix.add_argument("--ids", default=None, help="with --embed-plan: an .npy of token-id rows [N, L]")
    ix.add_argument("--mask", default=None, help="with --embed-plan: an .npy attention mask [N, L]")
    ix.add_argument("--images", default=None,
                    help="with a vision --embed-plan (ResNet / ViT): an .npy of uint8 images [N, H, W, 3] at the plan's "
                         "input size, or within its maximum for a resize plan")
    ix.add_argument("--labels", default=None, help="a JSON list of N strings")
    ix.add_argument("--tags", default=None, help="an .npy of N uint32 tag words (search filters test them): a version-2 file")
    ix.add_argument("--metric", choices=["cosine", "ip"], default="cosine")
    ix.add_argument("--pq-m", type=int, default=None, metavar="M",
                    help="with --dtype pq: code bytes per row (a multiple of 16 in 16..96 that divides dim; dim / M <= 64)")
    ix.add_argument("--pq-iters", type=int, default=None, help="with --dtype pq: Lloyd iterations of the codebook training (10)")
    ix.add_argument("--pq-seed", type=int, default=None, help="with --dtype pq: the training seed (0)")
    ix.add_argument("--pq-backend", choices=["cpu", "f32", "gpu"], default=None,
                    help="with --dtype pq: how training and encoding find the nearest sub-centroids: cpu (fp64 numpy, the "
                         "default), f32 (the GPU kernel's arithmetic in numpy) or gpu (HZ_K_SEARCH_PQASSIGN on --device; "
                         "the same bytes as f32)")
    ix.add_argument("--dtype", choices=["bf16", "fp8", "bin", "pq"], default="bf16",
                    help="fp8: e4m3fn rows with one fp32 scale per row (a version-3 file, half the bytes; D %% 16 == 0); "
                         "bin: one sign bit per column (a version-8 file, a sixteenth of the bytes; D %% 128 == 0), "
                         "with --rescore version 9")
    ix.add_argument("--rescore", action="store_true",
                    help="with --dtype fp8: also store the bf16 rows (a version-4 file) for two-stage search, "
                         "fp8 scan then exact bf16 re-scoring of the candidates")
    ix.add_argument("--ivf", type=int, default=None, metavar="NLIST",
                    help="an IVF index (a version-5 file; with --dtype fp8 version 6, with --rescore 7): the rows grouped "
                         "into NLIST k-means lists; a search scans the --nprobe lists nearest to the query")
    ix.add_argument("--nprobe", type=int, default=None, help="with --ivf: the lists a search scans by default (min(NLIST, 16))")
    ix.add_argument("--ivf-seed", type=int, default=None, help="with --ivf: the k-means seed (0)")
    ix.add_argument("--ivf-backend", choices=["cpu", "gpu"], default="cpu",
                    help="with --ivf: where k-means runs; gpu: Index.cluster on --device (dim %% 32 == 0)")
    ix.add_argument("--from-index", default=None, help="a bf16 .hzidx to rewrite in --dtype (rows requantised as stored, ids kept); an IVF file keeps its lists "
                         "(versions 6 and 7), --ivf NLIST builds lists over a plain file's stored rows")
    ix.add_argument("--model", default=None, help="free text kept in the header")
    ix.add_argument("--device", type=int, default=0)
    ix.add_argument("--out", required=True)
    kn = sub.add_parser("knn", help="the kNN graph of a plain bf16 .hzidx (dim %% 32 == 0): every live row's k nearest live rows")
    kn.add_argument("index", help="a .hzidx file")
    kn.add_argument("--k", type=int, default=10)
    kn.add_argument("--out", required=True, help="an .npz: ids int32 [count, k], scores float32 [count, k]")
    kn.add_argument("--backend", choices=["gpu", "cpu"], default="gpu")
    kn.add_argument("--block", type=int, default=None, help="rows per pass (default 1024)")
    kn.add_argument("--device", type=int, default=0)
    cl = sub.add_parser("cluster", help="k-means over the live rows of a plain bf16 .hzidx (dim %% 32 == 0)")
    cl.add_argument("index", help="a .hzidx file")
    cl.add_argument("--k", type=int, required=True, help="the number of clusters")
    cl.add_argument("--iters", type=int, default=10)
    cl.add_argument("--seed", type=int, default=0)
    cl.add_argument("--backend", choices=["gpu", "cpu"], default="gpu")
    cl.add_argument("--device", type=int, default=0)
    cl.add_argument("--out", required=True, help="an .npz: centroids uint16 [k, dim], assign int32 [count], score float32 [count]")
    inf = sub.add_parser("info")
    inf.add_argument("path", nargs="?", default=None, help="a .hzidx file: print its header")
    sub.add_parser("bench", add_help=False)
    args, rest = ap.parse_known_args(argv)
    if args.cmd == "bench":
        return cmd_bench(args, rest)
    {"serve": cmd_serve, "pack": cmd_pack, "plan": cmd_plan, "tune": cmd_tune, "upload": cmd_upload, "info": cmd_info,
     "index": cmd_index, "knn": cmd_knn, "cluster": cmd_cluster}[args.cmd](args)


if __name__ == "__main__":
    main()
