"""Bulk search over pq8 indexes on one GPU: ``Index.search_batch_pq(fallback=False)`` against the only
other route, ``Index.search`` over the same queries on the same index, in interleaved pairs; kind 50 alone beside kind
44 alone on bf16 rows of the same N; and the share of queries certified on a clustered and an isotropic corpus. Same
process, the first round warms up and captures, medians with min and max of the rest; every call returns with its results
in host memory, the kernels are timed with events.

    python scripts/bench_search_pqbatch.py [--n 100000 1000000] [--q 64 1024] [--m 96 48] [--dim 768] [--rounds 5]

The timing indexes hold the reconstructions of uniform random codes over a random codebook, encoded on the GPU (no
1e6-row corpus is trained); the certified shares come from codebooks trained on the corpus (``--certified-n`` rows).
Writes one JSON line per measurement to profiles/search_pqbatch/measure.jsonl (``--out`` elsewhere)."""
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
from scripts.bench_search_batch import corpus, med, timed  # noqa: E402


def kernels(codes, cb, q, R, rounds):
    """Kind 50 over the codes and kind 44 over the bf16 rows they decode to, each alone, timed with events."""
    import torch
    dev = "cuda:0"
    n, m = codes.shape
    Q, d = q.shape
    cb8 = S.pq_table_bf16(cb)
    bits = S.pq_decode_bf16(codes, cb8)
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(codes=codes, cb8=cb8.view(np.int16), rows=bits.view(np.int16), q=q).items()}
    nbytes = OS.self_scratch_bytes(n, Q, R)
    cand = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    s1, i1 = torch.empty((Q, R), dtype=torch.float32, device=dev), torch.empty((Q, R), dtype=torch.int32, device=dev)
    words = S.pack_live(np.ones(n, bool))
    lv = torch.from_numpy(words.view(np.int32)).to(dev)
    pq = OS.PqBatchScanParams(t["codes"].data_ptr(), t["q"].data_ptr(), lv.data_ptr(), cand.data_ptr(), s1.data_ptr(), i1.data_ptr(),
                              words.size * 4, nbytes, n, d, Q, R, m, 0, (C.c_int * 2)(), t["cb8"].data_ptr(), cb8.nbytes, m, 0)
    bf = OS.BatchScanParams(t["rows"].data_ptr(), t["q"].data_ptr(), lv.data_ptr(), cand.data_ptr(), s1.data_ptr(), i1.data_ptr(),
                            words.size * 4, nbytes, n, d, Q, R, d, 0)
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
    steps = (("pqxscan", N.HZ_K_SEARCH_PQXSCAN, pq), ("xscan", N.HZ_K_SEARCH_XSCAN, bf))
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
    ap.add_argument("--m", type=int, nargs="+", default=[96, 48])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--certified-n", type=int, default=100000, help="rows of the two trained corpora (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_pqbatch", "measure.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    R = S.batch_candidates(a.k)
    with tempfile.TemporaryDirectory() as tmp, open(a.out, "w") as f:
        def emit(**kw):
            f.write(json.dumps(kw) + "\n")
            f.flush()
            print(json.dumps(kw), flush=True)

        rng = np.random.default_rng(11)
        q_all = S.normalize_rows(rng.standard_normal((max(a.q), a.dim), dtype=np.float32))
        for n in a.n:
            for m in a.m:
                cb = (rng.standard_normal((m, 256, a.dim // m), dtype=np.float32) / np.float32(np.sqrt(a.dim)))
                codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
                path = os.path.join(tmp, f"r_{n}_{m}.hzidx")
                S.write_index(path, S.pq_decode(codes, cb), "ip", dtype="pq", pq_m=m, pq_codebook=cb, pq_backend="gpu")
                with S.Index(path) as ix:
                    for nq in a.q:
                        q = q_all[:nq]
                        t = {"search_batch_pq": [], "search": []}
                        for r in range(a.rounds + 1):  # interleaved pairs; the first round captures the programs
                            took = {"search_batch_pq": timed(lambda: ix.search_batch_pq(q, a.k, fallback=False)),
                                    "search": timed(lambda: ix.search(q, a.k))}
                            if r:
                                for name, v in took.items():
                                    t[name].append(v)
                        wins = sum(x < y for x, y in zip(t["search_batch_pq"], t["search"]))
                        for name, v in t.items():
                            emit(what=name, N=n, M=m, Q=nq, D=a.dim, k=a.k, R=R, pairs_won=wins, **med(v))
                        emit(what="kernels", N=n, M=m, Q=nq, D=a.dim, R=R, **kernels(S.read_rows(path), cb, q, R, a.rounds))
        for kind in ("clustered", "isotropic") if a.certified_n else ():
            rows, q = corpus(a.certified_n, a.dim, kind, 7, max(a.q))
            for m in a.m:
                path = os.path.join(tmp, f"{kind}_{m}.hzidx")
                S.write_index(path, rows, "cosine", dtype="pq", pq_m=m, pq_backend="gpu", pq_means="gpu")
                with S.Index(path) as ix:
                    s, i, certain = ix.search_batch_pq(q, a.k, fallback=False)
                    ws, wi = ix.search(q, a.k)
                    agree = bool(np.array_equal(i[certain], wi[certain]) and
                                 np.array_equal(s[certain].view(np.uint32), ws[certain].view(np.uint32)))
                    emit(what="certified", corpus=kind, N=a.certified_n, M=m, Q=len(q), D=a.dim, k=a.k, R=R,
                         share=round(float(certain.mean()), 4), equal_where_certain=agree,
                         ids_equal_share=round(float((i == wi).all(axis=1).mean()), 4))


if __name__ == "__main__":
    main()
