#!/usr/bin/env python3
"""The two measurements of profiles/resnet_embed/README.md on one MI355X, as JSON lines.

1. ``pool_norm_kernel`` alone, launch to launch, at (B1, HW49, C2048): the blocked bf16 input and the
   pooled fp32 input, ``pool_fc_kernel`` (1000 classes) on the same inputs next to them; rounds alternate
   the four, each round times ``--launches`` back-to-back launches with device events.
2. ResNet-50 bs=1, uint8 request, one context: the embedding program against the classification program
   of the same checkpoint, ``--pairs`` interleaved pairs. Per pair and program: the captured replay loop
   (``Engine.bench``, us per replay) and the single-request latency p50 of ``--requests`` ``infer`` calls
   sent one at a time (host wall: request copy, replay, wait, vector / logits out)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap.engine.engine import Engine  # noqa: E402
from hipzap.models import registry  # noqa: E402
from hipzap.models.resnet import randomize_bn  # noqa: E402
from hipzap.ops import vision as V  # noqa: E402
from hipzap.ops.conv import pack_linear, to_blocked  # noqa: E402

DEV = "cuda:0"


def _opt(flag, default):
    return int(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def _time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per launch


def kernel(rounds, launches):
    B, HW, Cc = 1, 49, 2048
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, 7, 7, Cc, generator=g) + 0.25).to(torch.bfloat16)
    xb = to_blocked(x.to(DEV))
    means = V.pool_norm(xb, False, blocked_input=True).contiguous()
    out = torch.empty(B, Cc, device=DEV)
    pc = pack_linear(torch.randn(1000, Cc, generator=g) * 0.02, torch.zeros(1000))
    pc.wf, pc.bias = pc.wf.to(DEV), pc.bias.to(DEV)
    logits = torch.empty(B, 1000, device=DEV)
    fc = {p: V.PoolFcParams(src.data_ptr(), pc.wf.data_ptr(), pc.bias.data_ptr(), logits.data_ptr(), B, Cc, HW, 1000,
                            1000, p) for p, src in ((0, xb), (1, means))}
    import ctypes as C
    from hipzap import _native as N
    pn = {p: V.PoolNormParams(src.data_ptr(), out.data_ptr(), B, Cc, HW, Cc, p, 1) for p, src in ((0, xb), (1, means))}
    launch, st = N.lib().hz_launch_kernel, N.stream_ptr()  # bound parameter blocks: the loop is one ctypes call per launch
    fns = {"pool_norm_blocked": lambda: launch(N.HZ_K_POOL_NORM, C.byref(pn[0]), st),
           "pool_norm_pooled": lambda: launch(N.HZ_K_POOL_NORM, C.byref(pn[1]), st),
           "pool_fc_blocked": lambda: launch(N.HZ_K_POOL_FC, C.byref(fc[0]), st),
           "pool_fc_pooled": lambda: launch(N.HZ_K_POOL_FC, C.byref(fc[1]), st)}
    ref = V.pool_norm_ref(x, True)
    for name in ("pool_norm_blocked", "pool_norm_pooled"):
        fns[name]()
        torch.cuda.synchronize()
        assert (out.double().cpu() - ref).abs().max() < 1e-6, name
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(_time(fn, launches))
    return {"what": "kernel", "B": B, "HW": HW, "C": Cc, "rounds": rounds, "launches_per_round": launches,
            **{f"{k}_us": [round(v, 2) for v in vs] for k, vs in us.items()},
            **{f"{k}_us_median": round(statistics.median(vs), 2) for k, vs in us.items()}}


def _p50_latency(eng, x, n):
    lat = []
    for _ in range(n + 10):
        t = time.perf_counter()
        eng.infer(x)
        lat.append((time.perf_counter() - t) * 1e6)
    return statistics.median(lat[10:])


def end_to_end(pairs, iters, requests):
    torch.manual_seed(0)
    sd = randomize_bn(registry.get("resnet50").make_model()).eval().state_dict()
    kw = dict(batch=1, num_contexts=1, zero_copy="all")
    cls = Engine.from_state_dict("resnet50", sd, DEV, arch_kw={"input_uint8": True}, **kw)
    emb = Engine.from_state_dict("resnet50", sd, DEV, arch_kw={"input_uint8": True, "head": "embed"}, **kw)
    x = torch.randint(0, 256, (1, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    for e in (cls, emb):
        e.bench(200)
        e.infer(x)
    c, m, cl, ml = [], [], [], []
    for _ in range(pairs):
        c.append(cls.bench(iters) / iters * 1e6)
        m.append(emb.bench(iters) / iters * 1e6)
        cl.append(_p50_latency(cls, x, requests))
        ml.append(_p50_latency(emb, x, requests))
    r = lambda vs: [round(v, 2) for v in vs]  # noqa: E731
    return {"what": "resnet50_bs1", "pairs": pairs, "iters_per_run": iters, "requests_per_run": requests,
            "ops": {"cls": cls.contexts[0].num_ops(), "embed": emb.contexts[0].num_ops()},
            "replay_us": {"cls": r(c), "embed": r(m)}, "latency_p50_us": {"cls": r(cl), "embed": r(ml)},
            "replay_us_median": {"cls": round(statistics.median(c), 2), "embed": round(statistics.median(m), 2)},
            "latency_p50_us_median": {"cls": round(statistics.median(cl), 2), "embed": round(statistics.median(ml), 2)},
            "replay_ratio_embed_over_cls": round(statistics.median(m) / statistics.median(c), 4),
            "latency_ratio_embed_over_cls": round(statistics.median(ml) / statistics.median(cl), 4)}


if __name__ == "__main__":
    print(json.dumps(kernel(_opt("--rounds", 7), _opt("--launches", 2000))), flush=True)
    if "--kernel-only" in sys.argv:
        sys.exit(0)
    print(json.dumps(end_to_end(_opt("--pairs", 7), _opt("--iters", 2000), _opt("--requests", 300))), flush=True)
