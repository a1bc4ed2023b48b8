"""Measure the resize plans on the GPU: the fused resize + crop + normalise kernel
alone, a ResNet-50 resize plan's single-stream latency, and its served rate next to the fixed-shape
plan of the same weights, interleaved on one box.

    python scripts/bench_resize.py [--out profiles/resize] [--contexts 12] [--clients 16]

* kernel: device events around a loop of back-to-back launches (after a warm-up of the same shape),
  the source read zero-copy from pinned host memory, as served, and from device memory;
* single stream: host clock around ``infer_image`` / ``infer_raw`` (each ends in the request's
  completion), one context, p50 over the loop;
* served: ``clients`` Python request threads through the native executor (the GIL is released inside
  a submit), fixed / resize alternating, three rounds each. Both plans go through the same Python
  client loop, so the two rates compare with each other; the fixed plan's headline rate (bench.py)
  uses native client threads and is higher.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hipzap import _native as N  # noqa: E402
from hipzap.engine.plan import export_plan  # noqa: E402
from hipzap.lite import PlanEngine  # noqa: E402
from hipzap.models import registry  # noqa: E402
from hipzap.models.resnet import randomize_bn  # noqa: E402
from hipzap.ops import vision as V  # noqa: E402

MAX = (1024, 1024)


def kernel_times(iters: int) -> dict:
    out = {}
    dst = torch.empty(1, 224, 224, 8, device="cuda", dtype=torch.bfloat16)
    for hw in [(500, 375), (1024, 1024)]:
        img = torch.randint(0, 256, (*hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        buf, dims = V.pack_images([img], 256, 224, *MAX)
        for where, b, d in (("pinned_host", buf.pin_memory(), dims.pin_memory()), ("device", buf.cuda(), dims.cuda())):
            prm = V.resize_params(b.data_ptr(), d.data_ptr(), dst.data_ptr(), 1, 224, *MAX, V.IMAGENET_MEAN,
                                  V.IMAGENET_STD)
            st = N.stream_ptr()
            launch = lambda: N.check(N.lib().hz_launch_kernel(N.HZ_K_RESIZE_PREPROCESS, C.byref(prm), st), "rz")  # noqa: E731
            for _ in range(50):
                launch()
            torch.cuda.synchronize()
            reps = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    launch()
                e1.record()
                e1.synchronize()
                reps.append(e0.elapsed_time(e1) * 1e3 / iters)
            out[f"{hw[0]}x{hw[1]}_{where}_us"] = {"median": round(statistics.median(reps), 2),
                                                  "min": round(min(reps), 2), "max": round(max(reps), 2),
                                                  "source_bytes": img.numel()}
    return out


def p50_ms(fn, iters: int) -> float:
    for _ in range(50):
        fn()
    lat = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(lat), 4)


def served_rate(fn, clients: int, iters: int) -> float:
    def work():
        for _ in range(iters):
            fn()
    th = [threading.Thread(target=work) for _ in range(clients)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return clients * iters / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/resize")
    ap.add_argument("--contexts", type=int, default=12)
    ap.add_argument("--clients", type=int, default=16)
    ap.add_argument("--iters", type=int, default=1500)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resize needs a GPU")
    res = {"gpu": torch.cuda.get_device_name(0), "max_image": list(MAX), "kernel": kernel_times(1000)}
    torch.manual_seed(0)
    ad = registry.get("resnet50")
    params, kw = ad.pack(randomize_bn(ad.make_model()).eval().state_dict(), "cpu")
    tmp = tempfile.mkdtemp()
    fixed, rz = os.path.join(tmp, "fixed.hzplan"), os.path.join(tmp, "rz.hzplan")
    export_plan("resnet50", params, dict(kw, input_uint8=True), fixed, batch=1, contexts=a.contexts)
    export_plan("resnet50", params, dict(kw, resize=[256, 224, *MAX]), rz, batch=1, contexts=a.contexts)
    g = np.random.default_rng(0)
    img224 = g.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    img500 = g.integers(0, 256, (375, 500, 3), dtype=np.uint8)
    img1024 = g.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    e_fixed, e_rz = PlanEngine(fixed, contexts=1), PlanEngine(rz, contexts=1)
    res["single_stream_p50_ms"] = {
        "fixed_224x224": p50_ms(lambda: e_fixed.infer_raw(img224), a.iters),
        "resize_375x500": p50_ms(lambda: e_rz.infer_image(img500), a.iters),
        "resize_1024x1024": p50_ms(lambda: e_rz.infer_image(img1024), a.iters),
        "fixed_224x224_again": p50_ms(lambda: e_fixed.infer_raw(img224), a.iters),
    }
    e_fixed.close()
    e_rz.close()
    s_fixed, s_rz = PlanEngine(fixed, contexts=a.contexts), PlanEngine(rz, contexts=a.contexts)
    rounds = []
    for _ in range(3):  # interleaved: fixed, resize 375x500, resize 1024x1024
        rounds.append({
            "fixed_224x224": round(served_rate(lambda: s_fixed.infer_raw(img224), a.clients, a.iters)),
            "resize_375x500": round(served_rate(lambda: s_rz.infer_image(img500), a.clients, a.iters)),
            "resize_1024x1024": round(served_rate(lambda: s_rz.infer_image(img1024), a.clients, a.iters // 3)),
        })
    res["served_req_per_s"] = {"contexts": a.contexts, "python_client_threads": a.clients, "rounds": rounds}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_resize.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
