"""Measurements for DESIGN.md 4s (neighbours of stored rows): ``Index.knn_graph`` against the only route the search
stack had for the same job -- ``Index.search`` over the widened rows, 16 a launch --, and one pass of the self scan and
its merge against ``torch.topk(c @ c[ids].T)`` in bf16. Same process, interleaved rounds, medians, launch to launch
(each call returns with its results on the host).

    python scripts/search_neighbors_measure.py --out profiles/search_neighbors/measure.jsonl
    python scripts/search_neighbors_measure.py --profile     # one small pass of each, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hipzap import search as S  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def graph_by_search(ix, rows32, k):
    """The parent's route: every row as an fp32 query, k + 1 hits, the self hit dropped on the host."""
    n = rows32.shape[0]
    ids = np.empty((n, k), np.int32)
    for a in range(0, n, 4096):
        s, i = ix.search(rows32[a:a + 4096], k + 1)
        for r in range(i.shape[0]):
            ids[a + r] = i[r][i[r] != a + r][:k]
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="one knn_graph and one search-route pass at the first --n, nothing timed")
    a = ap.parse_args()
    import torch
    lines = []
    for n in a.n:
        rng = np.random.default_rng(n)
        v = rng.standard_normal((n, a.dim)).astype(np.float32)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "c.hzidx")
            S.write_index(path, v, "cosine")
            rows32 = S.bf16_to_f32(S.read_rows(path))
            with S.Index(path) as ix:
                g0 = ix.knn_graph(a.k)[0]  # warm: programs captured
                if a.profile:
                    graph_by_search(ix, rows32[:4096], a.k)
                    return
                b0 = graph_by_search(ix, rows32[:2048], a.k)
                same = float((b0 == g0[:2048]).all(axis=1).mean())
                tg, tb = [], []
                base_rows = min(n, 20000)  # the search route is timed on a slice and scaled: it is linear in the queries
                for _ in range(a.rounds):
                    tg.append(timed(lambda: ix.knn_graph(a.k))[0])
                    tb.append(timed(lambda: ix.search(rows32[:base_rows], a.k + 1))[0] * n / base_rows)  # the searches alone
                lines.append({"what": "knn_graph", "n": n, "dim": a.dim, "k": a.k, "rounds": a.rounds,
                              "neighbors_ms": round(statistics.median(tg), 2), "search_route_ms": round(statistics.median(tb), 2),
                              "search_route_timed_rows": base_rows, "speedup": round(statistics.median(tb) / statistics.median(tg), 2),
                              "rows_with_equal_lists": same})
                c = torch.from_numpy(S.read_rows(path).view(np.int16)).cuda().view(torch.bfloat16)
                for q in (64, 1024):
                    ids = rng.permutation(n)[:q].astype(np.int32)
                    idt = torch.from_numpy(ids.astype(np.int64)).cuda()
                    ix.neighbors(ids, a.k, include_self=True)
                    torch.topk(c @ c[idt].T, a.k, dim=0)
                    tn, tt = [], []
                    for _ in range(a.rounds):
                        tn.append(timed(lambda: ix.neighbors(ids, a.k, include_self=True))[0])

                        def ref():
                            s, i = torch.topk((c @ c[idt].T).T, a.k, dim=1)
                            return s.float().cpu(), i.cpu()
                        tt.append(timed(ref)[0])
                    lines.append({"what": "one_pass", "n": n, "dim": a.dim, "k": a.k, "q": q,
                                  "neighbors_ms": round(statistics.median(tn), 3), "torch_bf16_topk_ms": round(statistics.median(tt), 3)})
                del c
        for ln in lines[-3:]:
            print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
