"""Product-quantisation training with the means on the GPU (HZ_K_SEARCH_PQUPDATE, ``hz_pq_train``, ``pq_train(backend=
"gpu", means="gpu")``) beside the path it replaces (``backend="gpu", means="host"``: the assignment on the GPU, the
means in numpy) on the same host in the same run (profiles/search_pqtrain/README.md).

    python scripts/bench_search_pqtrain.py --out profiles/search_pqtrain/search_pqtrain.json
    python scripts/bench_search_pqtrain.py --large 1000000 --rounds 0 --out profiles/search_pqtrain/large.json

  * train: wall time of ``pq_train`` over ``--rows`` x 768 rows, ``--iters`` iterations, for each ``--m``: (a) means on
    the host, then (b) means on the GPU, one pair per round -- every copy, the sampling and the bf16 check included;
    ``pairs_b_faster`` counts the rounds in which (b) took less time than (a);
  * kernel: device events around ``--reps`` launches of kind 48 and of kind 49 over rows already on the device, the
    codes those of kind 48 against the first centroids: the device work of one iteration;
  * large (``--large N``): ONE ``pq_train(sample=N, backend="gpu", means="gpu")`` over N x 768 rows at M = 96, its wall
    time, and ``pq_distortion`` of that codebook and of the ``--rows``-row one on 10,000 rows outside both samples.

Rounds are interleaved and medians are reported with the min-max spread. Rows are isotropic unit vectors rounded to
bf16."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

D, HELD_OUT = 768, 10000


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--m", type=int, nargs="+", default=[96, 48])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--large", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_search_pqtrain: no GPU; nothing is measured without one")
    dev = "cuda:0"
    total = max(a.rows, a.large) + HELD_OUT
    parts = []
    g = torch.Generator(device=dev).manual_seed(D)
    for at in range(0, total, 1 << 18):  # in pieces: the fp32 normals of 1e6 rows need not exist at once
        x = torch.randn((min(1 << 18, total - at), D), generator=g, device=dev)
        parts.append((x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16))
    rows_dev = torch.cat(parts).contiguous()
    del parts, x
    bits = rows_dev.view(torch.int16).cpu().numpy().view(np.uint16)
    held = S.bf16_to_f32(bits[-HELD_OUT:])
    small = S.bf16_to_f32(bits[:a.rows])
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": a.rows, "iters": a.iters,
           "train": {}, "kernel": {}, "pairs_b_faster": {}, "large": {}}
    acc = {}

    def note(group, key, value):
        acc.setdefault((group, key), []).append(value)

    def train(m, means):
        t = time.perf_counter()
        cb = S.pq_train(small, m, iters=a.iters, backend="gpu", means=means)
        return time.perf_counter() - t, cb

    def kernels(m):
        cb = torch.from_numpy(np.ascontiguousarray(small[:256].reshape(256, m, D // m).transpose(1, 0, 2))).to(dev)
        out = torch.empty_like(cb)
        codes = torch.empty((a.rows, m), dtype=torch.uint8, device=dev)
        pa = OS.PqAssignParams(rows_dev.data_ptr(), cb.data_ptr(), codes.data_ptr(), 0, 0, a.rows, D, m, D, m)
        pu = OS.PqUpdateParams(rows_dev.data_ptr(), codes.data_ptr(), cb.data_ptr(), out.data_ptr(), 0, a.rows, D, m, D, m)
        st = torch.cuda.current_stream().cuda_stream
        took = []
        for launch, p in ((OS.launch_pq_assign, pa), (OS.launch_pq_update, pu)):
            assert launch(p, st) == 0  # warm; the assign launch also writes the codes the update reads
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                assert launch(p, st) == 0
            e1.record()
            torch.cuda.synchronize()
            took.append(e0.elapsed_time(e1) / a.reps * 1e-3)
        return took

    OS.pq_train_rows(bits[:1024], np.zeros((96, 256, 8), np.float32), 1)  # the first call of a process loads the code
    for rnd in range(a.rounds):
        for m in a.m:
            ta, cba = train(m, "host")
            tb, cbb = train(m, "gpu")
            note("train", f"M={m} (a) means=host", ta)
            note("train", f"M={m} (b) means=gpu", tb)
            note("train", f"M={m} a/b", ta / tb)
            res["pairs_b_faster"][f"M={m}"] = res["pairs_b_faster"].get(f"M={m}", 0) + int(tb < ta)
            if rnd == 0:  # unit-norm rows: every fp64 sum is exact, so the two orders give the same codebook
                res["train"][f"M={m} same codebook"] = bool(np.array_equal(cba, cbb))
            k48, k49 = kernels(m)
            note("kernel", f"M={m} kind 48 (assign)", k48)
            note("kernel", f"M={m} kind 49 (update)", k49)
        print(f"round {rnd} done", flush=True)
    for (group, key), xs in acc.items():
        res[group][key] = summary(xs)
    if a.large:
        big = S.bf16_to_f32(bits[:a.large])
        t = time.perf_counter()
        cb = S.pq_train(big, 96, iters=a.iters, sample=a.large, backend="gpu", means="gpu")
        res["large"] = {"rows": a.large, "M": 96, "iters": a.iters, "seconds": time.perf_counter() - t}
        t = time.perf_counter()
        job = OS.pq_train_rows(bits[:a.large], cb, a.iters)  # the batch job alone: no sampling, no bf16 check
        res["large"]["hz_pq_train seconds"] = time.perf_counter() - t
        del job
        res["large"]["distortion, held-out rows"] = S.pq_distortion(held, cb)
        res["large"][f"distortion of the {a.rows}-row codebook"] = S.pq_distortion(
            held, S.pq_train(small, 96, iters=a.iters, backend="gpu", means="gpu"))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
