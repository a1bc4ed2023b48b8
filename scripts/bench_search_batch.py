"""Bulk search on one GPU: ``Index.search_batch`` against ``Index.search`` on the same queries (the
route it replaces) and one ``Index.neighbors`` pass of the same Q (the floor its two extra MFMA rounds sit on), the
per-kernel split of one call, and the share of queries certified without fallback on a clustered and an isotropic
corpus. Same process, interleaved rounds, medians; every call returns with its results in host memory.

    python scripts/bench_search_batch.py [--n 100000 1000000] [--q 64 1024 10000] [--dim 768] [--k 10] [--rounds 7]

Writes one JSON line per measurement to profiles/search_batch/measure.jsonl (``--out`` elsewhere)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hipzap import _native as N  # noqa: E402
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402


def corpus(n, d, kind, seed, nq):
    """-> (rows fp32 [n, d], queries fp32 [nq, d], unit length). "clustered": sqrt(n) centres, rows and queries at
    0.35 sigma around them; "isotropic": N(0, 1) rows and queries."""
    rng = np.random.default_rng(seed)
    if kind == "clustered":
        c = max(2, int(n ** 0.5))
        cent = rng.standard_normal((c, d), dtype=np.float32)
        rows = cent[rng.integers(0, c, n)] + np.float32(0.35) * rng.standard_normal((n, d), dtype=np.float32)
        q = cent[rng.integers(0, c, nq)] + np.float32(0.35) * rng.standard_normal((nq, d), dtype=np.float32)
    else:
        rows = rng.standard_normal((n, d), dtype=np.float32)
        q = rng.standard_normal((nq, d), dtype=np.float32)
    return rows, S.normalize_rows(q)


def med(times):
    return {"median_ms": round(statistics.median(times) * 1e3, 4), "min_ms": round(min(times) * 1e3, 4),
            "max_ms": round(max(times) * 1e3, 4), "rounds": len(times)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def kernel_split(ix_path, q, k, R, rounds):
    """Kinds 44, 40 and 45 launched one by one over device copies of the index's rows, each timed with events."""
    import torch
    bits = S.read_rows(ix_path)
    n, d = bits.shape
    dev = "cuda:0"
    corpus_d = torch.from_numpy(bits.view(np.int16)).to(dev)
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    Q = q.shape[0]
    nbytes = OS.self_scratch_bytes(n, Q, R)
    cand = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    s1, i1 = torch.empty((Q, R), dtype=torch.float32, device=dev), torch.empty((Q, R), dtype=torch.int32, device=dev)
    s2, i2 = torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int32, device=dev)
    words = S.pack_live(np.ones(n, bool))
    lv = torch.from_numpy(words.view(np.int32)).to(dev)
    bp = OS.BatchScanParams(corpus_d.data_ptr(), qd.data_ptr(), lv.data_ptr(), cand.data_ptr(), s1.data_ptr(), i1.data_ptr(),
                            words.size * 4, nbytes, n, d, Q, R, d, 0)
    rp = OS.RescoreParams(corpus_d.data_ptr(), qd.data_ptr(), i1.data_ptr(), s2.data_ptr(), i2.data_ptr(), n, d, Q, R, k, d)
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
    steps = (("xscan", N.HZ_K_SEARCH_XSCAN, bp), ("mergen", N.HZ_K_SEARCH_MERGEN, bp), ("rescoren", N.HZ_K_SEARCH_RESCOREN, rp))
    out = {name: [] for name, _, _ in steps}
    for r in range(rounds + 1):
        for name, kind, prm in steps:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = lib.hz_launch_kernel(kind, C.byref(prm), st)
            b.record()
            torch.cuda.synchronize()
            assert rc == 0, (name, rc)
            if r:  # the first round warms up
                out[name].append(a.elapsed_time(b) * 1e-3)
    return {name: med(t) for name, t in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--q", type=int, nargs="+", default=[64, 1024, 10000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_batch", "measure.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    R = S.batch_candidates(a.k)
    with tempfile.TemporaryDirectory() as tmp:
        for n in a.n:
            for kind in ("clustered", "isotropic"):
                rows, q_all = corpus(n, a.dim, kind, 7, max(a.q))
                path = os.path.join(tmp, f"{kind}_{n}.hzidx")
                S.write_index(path, rows, "cosine")
                del rows
                with S.Index(path) as ix:
                    for nq in a.q:
                        q = q_all[:nq]
                        s, i, certain = ix.search_batch(q, a.k, fallback=False)
                        ws, wi = ix.search(q, a.k)
                        agree = bool(np.array_equal(i[certain], wi[certain]) and
                                     np.array_equal(s[certain].view(np.uint32), ws[certain].view(np.uint32)))
                        emit(what="certified", corpus=kind, N=n, Q=nq, D=a.dim, k=a.k, R=R, share=round(float(certain.mean()), 4),
                             equal_where_certain=agree, ids_equal_share=round(float((i == wi).all(axis=1).mean()), 4))
                        if kind != "clustered":
                            continue
                        ids = np.arange(min(nq, n), dtype=np.int32)
                        t = {"search_batch": [], "search_batch_no_fallback": [], "search": [], "neighbors": []}
                        for r in range(a.rounds + 1):  # interleaved; the first round captures the programs
                            took = {"search_batch": timed(lambda: ix.search_batch(q, a.k)),
                                    "search_batch_no_fallback": timed(lambda: ix.search_batch(q, a.k, fallback=False)),
                                    "search": timed(lambda: ix.search(q, a.k)),
                                    "neighbors": timed(lambda: ix.neighbors(ids, a.k))}
                            if r:
                                for name, v in took.items():
                                    t[name].append(v)
                        for name, v in t.items():
                            emit(what=name, corpus=kind, N=n, Q=nq, D=a.dim, k=a.k, R=R, **med(v))
                    if kind == "clustered":
                        for nq, rr in ((min(1024, max(a.q)), R), (min(1024, max(a.q)), 128)):
                            emit(what="kernels", N=n, Q=nq, D=a.dim, k=a.k, R=rr, **{
                                name: v for name, v in kernel_split(path, q_all[:nq], a.k, rr, a.rounds).items()})
    with open(a.out, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
