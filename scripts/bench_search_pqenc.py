"""Product-quantisation training and encoding on the GPU (HZ_K_SEARCH_PQASSIGN, ``hz_pq_encode``, ``pq_train(backend=
"gpu")``) beside the numpy path (``backend="cpu"``) on the same host in the same run (DESIGN.md 4x,
profiles/search_pqenc/README.md).

    python scripts/bench_search_pqenc.py --out profiles/search_pqenc/search_pqenc.json

  * kernel: device events around ``--reps`` launches over rows already on the device, N x (D, M) as given;
  * encode: wall time of ``hz_pq_encode`` over host rows, every copy included;
  * train: ``pq_train`` over ``--train-rows`` x 768 rows, ``--train-iters`` iterations on the GPU, split into the time
    inside the assignment calls (device work and its copies) and the rest (the host's per-sub-space reduction);
  * host: ``pq_encode(backend="cpu")`` over ``--host-rows`` rows and ``pq_train(backend="cpu")`` at ``--host-iters``
    iterations (the numpy path costs the same every iteration; a figure for more iterations is an extrapolation).

Rounds are interleaved (every measurement once, then all again) and medians are reported with the min-max spread. Rows
are isotropic unit vectors rounded to bf16; a codebook is 256 of the rows. Operation counts: 3 * 256 * D fp32 operations
per row, N * D * 2 bytes of rows read, and N * 256 * D * 4 bytes of centroids read from LDS by each wave's lanes
together (one broadcast word serves 64 rows)."""
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


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--shapes", nargs="+", default=["768x96", "768x48", "768x16", "1024x16"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train-rows", type=int, default=65536)
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--train-m", type=int, nargs="+", default=[96, 48])
    ap.add_argument("--host-rows", type=int, default=100000)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_search_pqenc: no GPU; nothing is measured without one")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes]
    dev = "cuda:0"
    nmax = max(a.n + [a.train_rows, a.host_rows])
    rows_dev, rows_host, books = {}, {}, {}
    for d in sorted({d for d, _ in shapes} | {768}):
        g = torch.Generator(device=dev).manual_seed(d)
        x = torch.randn((nmax, d), generator=g, device=dev)
        rows_dev[d] = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
        rows_host[d] = rows_dev[d].view(torch.int16).cpu().numpy().view(np.uint16)
        del x
    for d, m in shapes + [(768, m) for m in a.train_m]:
        books[(d, m)] = np.ascontiguousarray(S.bf16_to_f32(rows_host[d][:256]).reshape(256, m, d // m).transpose(1, 0, 2))
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "kernel": {}, "encode": {}, "train": {},
           "host_encode": {}, "host_train": {}}
    acc = {}

    def note(group, key, value):
        acc.setdefault((group, key), []).append(value)

    def kernel(n, d, m):
        cb = torch.from_numpy(books[(d, m)]).to(dev)
        codes = torch.empty((n, m), dtype=torch.uint8, device=dev)
        p = OS.PqAssignParams(rows_dev[d].data_ptr(), cb.data_ptr(), codes.data_ptr(), 0, 0, n, d, m, d, m)
        st = torch.cuda.current_stream().cuda_stream
        assert OS.launch_pq_assign(p, st) == 0  # warm
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            assert OS.launch_pq_assign(p, st) == 0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e-3

    def train_gpu(m, iters):
        x = S.bf16_to_f32(rows_host[768][:a.train_rows])
        inside, inner = [0.0], S._pq_assign

        def timed(*args, **kw):
            t = time.perf_counter()
            out = inner(*args, **kw)
            inside[0] += time.perf_counter() - t
            return out
        S._pq_assign = timed
        try:
            t = time.perf_counter()
            S.pq_train(x, m, iters=iters, backend="gpu")
            total = time.perf_counter() - t
        finally:
            S._pq_assign = inner
        return total, inside[0]

    OS.pq_encode_rows(rows_host[768][:1024], books[(768, 96)])  # the first call of a process loads the code
    for rnd in range(a.rounds):
        for n in a.n:
            for d, m in shapes:
                note("kernel", f"N={n} D={d} M={m}", kernel(n, d, m))
                t = time.perf_counter()
                OS.pq_encode_rows(rows_host[d][:n], books[(d, m)])
                note("encode", f"N={n} D={d} M={m}", time.perf_counter() - t)
        for m in a.train_m:
            total, inside = train_gpu(m, a.train_iters)
            note("train", f"rows={a.train_rows} M={m} iters={a.train_iters} total", total)
            note("train", f"rows={a.train_rows} M={m} iters={a.train_iters} assign calls", inside)
            note("train", f"rows={a.train_rows} M={m} iters={a.train_iters} host reduction", total - inside)
            total, inside = train_gpu(m, a.host_iters)
            note("train", f"rows={a.train_rows} M={m} iters={a.host_iters} total", total)
        if rnd < a.host_rounds:
            for m in a.train_m:
                x = S.bf16_to_f32(rows_host[768][:a.host_rows])
                t = time.perf_counter()
                S.pq_encode(x, books[(768, m)])
                note("host_encode", f"N={a.host_rows} D=768 M={m}", time.perf_counter() - t)
                x = S.bf16_to_f32(rows_host[768][:a.train_rows])
                t = time.perf_counter()
                S.pq_train(x, m, iters=a.host_iters)
                note("host_train", f"rows={a.train_rows} M={m} iters={a.host_iters}", time.perf_counter() - t)
        print(f"round {rnd} done", flush=True)
    for (group, key), xs in acc.items():
        res[group][key] = summary(xs)
    for key, s in res["kernel"].items():  # achieved rates of the kernel alone
        n, d, m = (int(v.split("=")[1]) for v in key.split())
        s["fp32_ops_per_s"] = 3.0 * 256 * d * n / s["median"]
        s["lds_broadcast_bytes_per_s"] = 256.0 * d * 4 * (n / 64.0) / s["median"]
        s["row_bytes_per_s"] = 2.0 * d * n / s["median"]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
