"""Bulk search over fp8 indexes on one GPU: ``Index.search_batch_fp8(fallback=False)`` against the only
other route, ``Index.search`` over the same queries on the same index, in interleaved pairs; kind 52 alone beside kind
44 alone on the bf16 rows of the same N; and the share of queries certified on 4n's two corpora (isotropic Gaussian;
1,000 clusters, sigma 0.1, the queries drawn like the rows). Same process, the first round warms up and captures,
medians with min and max of the rest; every call returns with its results in host memory, the kernels are timed with
events.

    python scripts/bench_search_fp8batch.py [--n 100000 1000000] [--q 64 1024] [--dim 768] [--rounds 5]

The corpora are drawn and quantised on the GPU with torch (its float8_e4m3fn cast is ``to_e4m3`` bit for bit, DESIGN.md
4n; the host quantiser needs 100 s for 1e6 x 768). Writes one JSON line per measurement to
profiles/search_fp8batch/measure.jsonl (``--out`` elsewhere)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hipzap import _native as N  # noqa: E402
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402
from scripts.bench_search_batch import med, timed  # noqa: E402

DEV = "cuda:0"


def draw(n, d, kind, seed, nq):
    """-> (unit rows fp32 [n, d] on the device, unit queries fp32 [nq, d] on the host), the queries drawn like the rows."""
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((n + nq, d), generator=g, device=DEV)
    if kind == "clusters":
        cent = torch.randn((1000, d), generator=g, device=DEV)
        x = cent[torch.randint(0, 1000, (n + nq,), generator=g, device=DEV)] + 0.1 * x
    x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return x[:n], S.normalize_rows(x[n:].cpu().numpy())


def quantise(rows):
    """prepare_rows_fp8's arithmetic in torch -> (codes uint8 [n, d], scales fp32 [n]), both on the device."""
    import torch
    amax = rows.abs().amax(dim=1)
    scale = (amax / 448.0).clamp_min(float(np.finfo(np.float32).tiny))
    scale[amax == 0] = 1.0
    codes = (rows / scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, scale


def write(path, codes, scales):
    n, d = codes.shape
    hdr = {"dim": d, "count": n, "dtype": S.FP8, "metric": "cosine", "model": "", "embed": None}
    S._write_file(path, hdr, codes.cpu().numpy(), scales=scales.cpu().numpy())


def kernels(codes, scales, q, R, rounds):
    """Kind 52 over the codes and kind 44 over the bf16 rows ``scale * decode(code)`` rounded to bf16, each alone."""
    import torch
    n, d = codes.shape
    Q = q.shape[0]
    rows = (codes.view(torch.float8_e4m3fn).to(torch.float32) * scales[:, None]).to(torch.bfloat16)
    qd = torch.from_numpy(q).to(DEV)
    nbytes = OS.self_scratch_bytes(n, Q, R)
    cand = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    s1, i1 = torch.empty((Q, R), dtype=torch.float32, device=DEV), torch.empty((Q, R), dtype=torch.int32, device=DEV)
    words = S.pack_live(np.ones(n, bool))
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    q8 = OS.QuantBatchScanParams(codes.data_ptr(), qd.data_ptr(), lv.data_ptr(), cand.data_ptr(), s1.data_ptr(), i1.data_ptr(),
                                 words.size * 4, nbytes, n, d, Q, R, d, 0, (C.c_int * 2)(), scales.data_ptr(), 4 * n)
    bf = OS.BatchScanParams(rows.data_ptr(), qd.data_ptr(), lv.data_ptr(), cand.data_ptr(), s1.data_ptr(), i1.data_ptr(),
                            words.size * 4, nbytes, n, d, Q, R, d, 0)
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
    steps = (("qxscan", N.HZ_K_SEARCH_QXSCAN, q8), ("xscan", N.HZ_K_SEARCH_XSCAN, bf))
    out = {name: [] for name, _, _ in steps}
    for r in range(rounds + 1):
        for name, kind, prm in steps:  # interleaved
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = lib.hz_launch_kernel(kind, C.byref(prm), st)
            b.record()
            torch.cuda.synchronize()
            assert rc == 0, (name, rc)
            if r:
                out[name].append(a.elapsed_time(b) * 1e-3)
    return {name: med(v) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--q", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--certified-n", type=int, default=100000, help="rows of 4n's two corpora (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_fp8batch", "measure.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    R = S.batch_candidates(a.k)
    with tempfile.TemporaryDirectory() as tmp, open(a.out, "w") as f:
        def emit(**kw):
            f.write(json.dumps(kw) + "\n")
            f.flush()
            print(json.dumps(kw), flush=True)

        for n in a.n:
            rows, q_all = draw(n, a.dim, "isotropic", 11, max(a.q))
            codes, scales = quantise(rows)
            del rows
            path = os.path.join(tmp, f"r_{n}.hzidx")
            write(path, codes, scales)
            with S.Index(path) as ix:
                for nq in a.q:
                    q = q_all[:nq]
                    t = {"search_batch_fp8": [], "search": []}
                    for r in range(a.rounds + 1):  # interleaved pairs; the first round captures the programs
                        took = {"search_batch_fp8": timed(lambda: ix.search_batch_fp8(q, a.k, fallback=False)),
                                "search": timed(lambda: ix.search(q, a.k))}
                        if r:
                            for name, v in took.items():
                                t[name].append(v)
                    wins = sum(x < y for x, y in zip(t["search_batch_fp8"], t["search"]))
                    for name, v in t.items():
                        emit(what=name, N=n, Q=nq, D=a.dim, k=a.k, R=R, pairs_won=wins, **med(v))
                    emit(what="kernels", N=n, Q=nq, D=a.dim, R=R, **kernels(codes, scales, q, R, a.rounds))
            del codes, scales
        for kind in ("isotropic", "clusters") if a.certified_n else ():
            rows, q = draw(a.certified_n, a.dim, kind, 7, max(a.q))
            path = os.path.join(tmp, f"{kind}.hzidx")
            write(path, *quantise(rows))
            with S.Index(path) as ix:
                s, i, certain = ix.search_batch_fp8(q, a.k, fallback=False)
                ws, wi = ix.search(q, a.k)
                agree = bool(np.array_equal(i[certain], wi[certain]) and
                             np.array_equal(s[certain].view(np.uint32), ws[certain].view(np.uint32)))
                emit(what="certified", corpus=kind, N=a.certified_n, Q=len(q), D=a.dim, k=a.k, R=R,
                     share=round(float(certain.mean()), 4), equal_where_certain=agree,
                     ids_equal_share=round(float((i == wi).all(axis=1).mean()), 4))


if __name__ == "__main__":
    main()
