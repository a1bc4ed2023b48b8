"""Bulk search over binary indexes on one GPU: ``Index.search_batch_bin(refine=R)`` against the route
users had, ``Index.search(refine=R)`` in its parts of 16, on the same version-9 index in the same process, in
interleaved pairs; then kinds 59 (also over an all-dead bitmap: staging and barriers only; and at half and double the
launcher's span), 40 and 45 alone, timed with events. The first round warms up and captures; medians with min and max of
the rest. Every call returns with its results in host memory.

    python scripts/bench_search_binbatch.py [--n 100000 1000000] [--q 64 1024] [--refine 40 128] [--dim 768] [--rounds 5]

Writes one JSON line per measurement to profiles/search_binbatch/measure.jsonl (``--out`` elsewhere)."""
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


def kernels(path, q, k, R, rounds):
    """Kind 59 at the launcher's span (live and all-dead bitmaps), at half and double that span, kinds 40 and 45: each
    alone over device copies of the index's rows -> {name: times}, the span and the scratch bytes."""
    import torch
    words, rbits = S.read_rows(path), S.read_rescore_rows(path)
    n, w = words.shape
    Q, T = q.shape[0], OS.tile_rows()
    dw = torch.from_numpy(words.view(np.int32)).to(DEV)
    dr = torch.from_numpy(rbits.view(np.int16)).to(DEV)
    dq = torch.from_numpy(np.ascontiguousarray(q)).to(DEV)
    lw = S.pack_live(np.ones(n, bool))
    live, dead = torch.from_numpy(lw.view(np.int32)).to(DEV), torch.zeros(lw.size, dtype=torch.int32, device=DEV)
    span, ntile = OS.bin_batch_span(n, Q, R), -(-n // T)
    # the launcher's span runs last of the scans, so the merge that follows reads ITS lists: what the route merges
    spans = {"bxscan_dead": span, "bxscan_half_span": max(1, span // 2), "bxscan_double_span": min(ntile, 2 * span), "bxscan": span}
    nbytes = max(OS.bin_batch_scratch_bytes(n, Q, R, s) for s in spans.values())
    cand = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    s1, i1 = torch.empty((Q, R), dtype=torch.float32, device=DEV), torch.empty((Q, R), dtype=torch.int32, device=DEV)
    s2, i2 = torch.empty((Q, k), dtype=torch.float32, device=DEV), torch.empty((Q, k), dtype=torch.int32, device=DEV)
    steps = []
    for name, s in spans.items():
        lv = dead if name == "bxscan_dead" else live
        steps.append((name, N.HZ_K_SEARCH_BXSCAN, OS.BinBatchScanParams(
            dw.data_ptr(), dq.data_ptr(), lv.data_ptr(), cand.data_ptr(), s1.data_ptr(), i1.data_ptr(), lw.size * 4, nbytes,
            n, 32 * w, Q, R, w, 0, s, 0)))
    steps.append(("mergen", N.HZ_K_SEARCH_MERGEN, steps[-1][2].merge_params(-(-ntile // span))))
    steps.append(("rescoren", N.HZ_K_SEARCH_RESCOREN, OS.RescoreParams(dr.data_ptr(), dq.data_ptr(), i1.data_ptr(), s2.data_ptr(),
                                                                       i2.data_ptr(), n, 32 * w, Q, R, k, 32 * w)))
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
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
    return ({name: med(v) for name, v in out.items()}, span, OS.bin_batch_scratch_bytes(n, Q, R, span),
            OS.self_scratch_bytes(n, Q, R))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--q", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--refine", type=int, nargs="+", default=[40, 128])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_binbatch", "measure.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp, open(a.out, "w") as f:
        def emit(**kw):
            f.write(json.dumps(kw) + "\n")
            f.flush()
            print(json.dumps(kw), flush=True)

        for n in a.n:
            rng = np.random.default_rng(11)
            q_all = rng.standard_normal((max(a.q), a.dim), dtype=np.float32)
            path = os.path.join(tmp, f"b_{n}.hzidx")
            S.write_index(path, rng.standard_normal((n, a.dim), dtype=np.float32), "ip", dtype="bin", rescore=True)
            with S.Index(path) as ix:
                for nq in a.q:
                    q = q_all[:nq]
                    for R in a.refine:
                        t = {"search_batch_bin": [], "search": []}
                        for r in range(a.rounds + 1):  # interleaved pairs; the first round captures the programs
                            took = {"search_batch_bin": timed(lambda: ix.search_batch_bin(q, a.k, refine=R)),
                                    "search": timed(lambda: ix.search(q, a.k, refine=R))}
                            if r:
                                for name, v in took.items():
                                    t[name].append(v)
                        got, want = ix.search_batch_bin(q, a.k, refine=R), ix.search(q, a.k, refine=R)
                        same = bool(np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)))
                        wins = sum(x < y for x, y in zip(t["search_batch_bin"], t["search"]))
                        for name, v in t.items():
                            emit(what=name, N=n, Q=nq, D=a.dim, k=a.k, R=R, pairs_won=wins, equal=same, **med(v))
            for nq in a.q:
                for R in a.refine:
                    ks, span, slab_bytes, tile_bytes = kernels(path, q_all[:nq], a.k, R, a.rounds)
                    emit(what="kernels", N=n, Q=nq, D=a.dim, k=a.k, R=R, span=span, scratch_bytes=slab_bytes,
                         scratch_bytes_per_tile_lists=tile_bytes, **ks)


if __name__ == "__main__":
    main()
