"""Measure the ViT image plans on the GPU: the fused resize + patchify kernel next to
the NHWC8 resize kernel on the same inputs, and a ViT-B/16 request three ways, interleaved on one box.

    python scripts/bench_vit_image.py [--out profiles/resize_vit] [--iters 300]

* kernel: device events around a loop of back-to-back launches (after a warm-up of the same shape),
  the two kernels alternating rep by rep, the source read zero-copy from pinned host memory, as served,
  and from device memory;
* single stream (batch 1, one context, random weights), host clock around a call that ends in the
  request's completion, p50 over the loop, three rounds with the three paths alternating:
  ``resize_plan``  a 375x500 uint8 image into the resize plan (``PlanEngine.infer_image``),
  ``fixed_plan``   a ready fp32 NCHW tensor into the fixed-shape plan (``PlanEngine.infer_raw``),
  ``host_resize``  the same image resized, cropped and normalised on the host (the serving route's
                   ``to_model_input``) and run by the torch-built engine (``Engine.infer``).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hipzap import _native as N  # noqa: E402
from hipzap.engine.engine import Engine  # noqa: E402
from hipzap.engine.plan import export_plan  # noqa: E402
from hipzap.lite import PlanEngine  # noqa: E402
from hipzap.models import vit  # noqa: E402
from hipzap.ops import vision as V  # noqa: E402

MAX = (1024, 1024)


def kernel_times(iters: int) -> dict:
    out = {}
    nhwc = torch.empty(1, 224, 224, 8, device="cuda", dtype=torch.bfloat16)
    rows = torch.empty(196, 768, device="cuda", dtype=torch.bfloat16)
    st = N.stream_ptr()
    for hw in [(500, 375), (1024, 1024)]:
        img = torch.randint(0, 256, (*hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        buf, dims = V.pack_images([img], 256, 224, *MAX)
        for where, b, d in (("pinned_host", buf.pin_memory(), dims.pin_memory()), ("device", buf.cuda(), dims.cuda())):
            kinds = {"resize_preprocess": (N.HZ_K_RESIZE_PREPROCESS, nhwc),
                     "resize_patchify": (N.HZ_K_RESIZE_PATCHIFY, rows)}
            prms = {k: V.resize_params(b.data_ptr(), d.data_ptr(), dst.data_ptr(), 1, 224, *MAX, V.IMAGENET_MEAN,
                                       V.IMAGENET_STD) for k, (_, dst) in kinds.items()}

            def launch(k):
                N.check(N.lib().hz_launch_kernel(kinds[k][0], C.byref(prms[k]), st), k)

            reps = {k: [] for k in kinds}
            for k in kinds:
                for _ in range(50):
                    launch(k)
            torch.cuda.synchronize()
            for _ in range(5):
                for k in kinds:  # alternating
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        launch(k)
                    e1.record()
                    e1.synchronize()
                    reps[k].append(e0.elapsed_time(e1) * 1e3 / iters)
            for k, r in reps.items():
                out[f"{hw[0]}x{hw[1]}_{where}_{k}_us"] = {"median": round(statistics.median(r), 2),
                                                          "min": round(min(r), 2), "max": round(max(r), 2)}
    return out


def p50_ms(fn, iters: int) -> float:
    lat = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(lat), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/resize_vit")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--layers", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vit_image needs a GPU")
    from hipzap.serve.app import to_model_input
    res = {"gpu": torch.cuda.get_device_name(0), "max_image": list(MAX), "kernel": kernel_times(1000)}
    torch.manual_seed(0)
    sd = vit.make_model(num_hidden_layers=a.layers).state_dict()
    params, kw = vit.pack_vit(sd, "cpu")
    tmp = tempfile.mkdtemp()
    fixed, rz = os.path.join(tmp, "fixed.hzplan"), os.path.join(tmp, "rz.hzplan")
    export_plan("vit-b16", params, dict(kw), fixed, batch=1, contexts=1)
    export_plan("vit-b16", params, dict(kw, resize=[256, 224, *MAX]), rz, batch=1, contexts=1)
    img = np.random.default_rng(0).integers(0, 256, (375, 500, 3), dtype=np.uint8)
    spec = (256, 224, *MAX)
    x = to_model_input(img[None], spec).contiguous()
    e_fixed, e_rz = PlanEngine(fixed, contexts=1), PlanEngine(rz, contexts=1)
    eng = Engine.from_state_dict("vit-b16", sd, "cuda:0", batch=1, num_contexts=1)
    paths = {"resize_plan_375x500": lambda: e_rz.infer_image(img),
             "fixed_plan_ready_fp32": lambda: e_fixed.infer_raw(x),
             "host_resize_375x500_torch_engine": lambda: eng.infer(to_model_input(img[None], spec))}
    for fn in paths.values():
        for _ in range(30):
            fn()
    res["single_stream_p50_ms"] = {"layers": a.layers, "rounds": [{k: p50_ms(fn, a.iters) for k, fn in paths.items()}
                                                                  for _ in range(3)]}
    # the same request through the three paths: the plan's answer against the host path's
    y_rz = np.frombuffer(e_rz.infer_image(img), np.float32)
    y_host = eng.infer(x).numpy().reshape(-1)
    res["resize_plan_vs_host_path_max_abs_logit_diff"] = float(np.abs(y_rz[: y_host.size] - y_host).max())
    res["max_abs_logit"] = float(np.abs(y_host).max())
    e_fixed.close()
    e_rz.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_vit_image.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
