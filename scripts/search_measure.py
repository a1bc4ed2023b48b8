#!/usr/bin/env python3
"""The measurements of profiles/search/README.md on one MI355X; writes that file with its raw JSON.

1. scan + merge, launch to launch (device events around ``--launches`` back-to-back pairs), D = 768, k = 10,
   N in {1e4, 1e5, 1e6} x Q in {1, 16}, interleaved round by round with the reference
   ``torch.topk(q @ c.T, k)`` over the SAME bf16 corpus. torch gets the query in bf16 (its fast path:
   a bf16 GEMM); the kernel takes the fp32 query, as the index does.
2. POST /search against POST /embed, single stream, BERT-base bs1 (random weights, L = 16 tokens) with a
   1e5-row cosine index: Flask test client (no socket), interleaved rounds, p50 of the wall time per request.

    python scripts/search_measure.py [--out profiles/search] [--rounds 7] [--launches 50] [--no-serve]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

DEV = "cuda:0"
D, K = 768, 10


def _opt(flag, default, cast=int):
    return cast(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def _time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per call


def cell(N, Q, rounds, launches):
    g = torch.Generator(device=DEV).manual_seed(N + Q)
    corpus = torch.randn(N, D, generator=g, device=DEV).to(torch.bfloat16)
    q = torch.randn(Q, D, generator=g, device=DEV)
    q16 = q.to(torch.bfloat16)
    nbytes = OS.scratch_bytes(N, Q, K)
    cand = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    sc = torch.empty(Q, K, device=DEV)
    ids = torch.empty(Q, K, dtype=torch.int32, device=DEV)
    p = OS.SearchParams(corpus.data_ptr(), q.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                        N, D, Q, K, D, 0, nbytes)
    st = torch.cuda.current_stream().cuda_stream

    def hip():
        assert OS.launch(p, st) == (0, 0)

    def ref():
        return torch.topk(q16 @ corpus.T, K)

    hip()
    torch.cuda.synchronize()
    if N <= 10 ** 4:  # a sanity check of what is timed: the neighbours of an fp32 matmul over the same rows
        want = torch.topk(q @ corpus.float().T, K).indices.int()
        assert (want.sort(1).values == ids.sort(1).values).float().mean() > 0.95
    hs, ts = [], []
    for _ in range(rounds):
        hs.append(_time(hip, launches))
        ts.append(_time(ref, launches))
    h, t = statistics.median(hs), statistics.median(ts)
    return {"N": N, "Q": Q, "D": D, "k": K, "rounds": rounds, "launches_per_round": launches,
            "hip_us": [round(v, 1) for v in hs], "torch_us": [round(v, 1) for v in ts],
            "hip_us_median": round(h, 1), "torch_us_median": round(t, 1), "hip_over_torch": round(h / t, 3),
            "corpus_bytes": N * D * 2, "hip_read_TBps": round(N * D * 2 / h / 1e6, 3)}


def serve(rounds, requests):
    import tempfile

    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tempfile.mkdtemp(prefix="hz-search-")
    rng = np.random.default_rng(0)
    path = os.path.join(root, "c.hzidx")
    S.write_index(path, rng.standard_normal((10 ** 5, D)).astype(np.float32), "cosine")
    st = Settings(default_model="resnet18", artifact_root=root)
    st.models["bert-emb"] = ModelSpec(name="bert-base", key="random", batch=1, extra={
        "embed": {"pooling": "mean", "normalize": True}, "seq_len": 128, "index": path})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    body = {"model": "bert-emb", "input_ids": [rng.integers(1000, 30000, 16).tolist()], "k": K}
    hdr = {"Accept": "application/octet-stream"}
    out = {"embed_ms": [], "search_ms": []}
    with app_mod.app.test_client() as c:
        for route in ("/embed", "/search"):
            for _ in range(20):
                assert c.post(route, json=body, headers=hdr).status_code == 200
        for _ in range(rounds):
            for route, key in (("/embed", "embed_ms"), ("/search", "search_ms")):
                lat = []
                for _ in range(requests):
                    t0 = time.perf_counter()
                    c.post(route, json=body, headers=hdr)
                    lat.append((time.perf_counter() - t0) * 1e3)
                out[key].append(round(statistics.median(lat), 3))
    srv.close()
    app_mod.set_server(None)
    e, s = statistics.median(out["embed_ms"]), statistics.median(out["search_ms"])
    return {"what": "bert-base bs1, 16 tokens, 1e5-row cosine index, Flask test client, .npy answers",
            "rounds": rounds, "requests_per_round": requests, **out, "embed_p50_ms": round(e, 3),
            "search_p50_ms": round(s, 3), "search_minus_embed_ms": round(s - e, 3)}


def main():
    out_dir = _opt("--out", "profiles/search", str)
    rounds, launches = _opt("--rounds", 7), _opt("--launches", 50)
    os.makedirs(out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tile_rows": OS.tile_rows(), "cells": []}
    for N in (10 ** 4, 10 ** 5, 10 ** 6):
        for Q in (1, 16):
            res["cells"].append(cell(N, Q, rounds, launches))
            print(json.dumps(res["cells"][-1]), flush=True)
    if "--no-serve" not in sys.argv:
        res["serve"] = serve(5, 100)
        print(json.dumps(res["serve"]), flush=True)
    lines = ["# Vector search: scan + merge against torch.topk (scripts/search_measure.py)", "",
             f"Device: {res['device']}, torch {res['torch']}. D = {D}, k = {K}, tile = {res['tile_rows']} rows.",
             "Launch to launch, device events; medians over interleaved rounds. torch reference: "
             "`torch.topk(q @ c.T, k)` with a **bf16 query** over the same bf16 corpus (its fast path); the kernel "
             "takes the fp32 query.", "",
             "| N | Q | scan + merge (us) | torch (us) | ours / torch | corpus bytes / our time (TB/s) |", "|---|---|---|---|---|---|"]
    for c in res["cells"]:
        lines.append(f"| {c['N']} | {c['Q']} | {c['hip_us_median']} | {c['torch_us_median']} | {c['hip_over_torch']} | "
                     f"{c['hip_read_TBps']} |")
    if "serve" in res:
        s = res["serve"]
        lines += ["", f"POST /search against POST /embed ({s['what']}): p50 {s['search_p50_ms']} ms against "
                  f"{s['embed_p50_ms']} ms, a difference of {s['search_minus_embed_ms']} ms."]
    lines += ["", "Raw:", "", "```json", json.dumps(res, indent=1), "```", ""]
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
