"""Graph search against the exact scan and an IVF index of the same vectors: recall@10 against fp64
truth and milliseconds per call, launch to sync, the routes interleaved. ``--seeds`` adds per-query entry rows (4ae).

    python scripts/search_graph_measure.py --n 100000 --out profiles/search_graph/measure.jsonl
"""
import argparse
import contextlib
import json
import os
import tempfile
import time

import numpy as np

from hipzap import search as S


def corpus(kind, n, d, nq, rng):
    if kind == "isotropic":
        return rng.standard_normal((n, d), np.float32), rng.standard_normal((nq, d), np.float32)
    cent = rng.standard_normal((1024, d), np.float32)
    return (cent[rng.integers(0, 1024, n)] + rng.standard_normal((n, d), np.float32),
            cent[rng.integers(0, 1024, nq)] + rng.standard_normal((nq, d), np.float32))


def recall(ids, truth):
    return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids, truth)) / truth.size


def prune_kernel_ms(knn, launches=20):
    """HZ_K_GRAPH_PRUNE alone over device lists: device events around ``launches`` back-to-back launches after a warm-up
    one, milliseconds per launch."""
    import torch
    from hipzap.ops import search as OS
    src = torch.from_numpy(np.ascontiguousarray(knn, np.int32)).to("cuda:0")
    order, det = torch.empty_like(src), torch.empty_like(src)
    p = OS.GraphPruneParams(src.data_ptr(), order.data_ptr(), det.data_ptr(), *knn.shape)
    st = torch.cuda.current_stream().cuda_stream
    assert OS.launch_graph_prune(p, st) == 0
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        OS.launch_graph_prune(p, st)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / launches


def seed_kernel_ms(ix, q, E, launches=20):
    """HZ_K_GRAPH_SEED alone, over device copies of the index's rows, ``q`` and its seed table: device events around ``launches`` back-to-back launches after a
    warm-up one, milliseconds per launch."""
    import torch
    from hipzap.ops import search as OS
    bits = S.read_rows(ix.path)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (bits.view(np.int16), np.ascontiguousarray(q, np.float32), ix.graph_seed_table)]
    out = torch.empty((q.shape[0], E), dtype=torch.int32, device="cuda:0")
    p = OS.GraphSeedParams(*(t.data_ptr() for t in dev), out.data_ptr(), bits.shape[0], bits.shape[1], q.shape[0],
                           ix.graph_seed_table.size, E, bits.shape[1], E)
    st = torch.cuda.current_stream().cuda_stream
    assert OS.launch_graph_seed(p, st) == 0
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        OS.launch_graph_seed(p, st)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--deg", type=int, default=32)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--truth-queries", type=int, default=256)
    ap.add_argument("--out", default="search_graph.jsonl")
    ap.add_argument("--prune", action="store_true",
                    help="add the pruned graph (DESIGN.md 4ad): its build time, its search_graph rows, HZ_K_GRAPH_PRUNE's time")
    ap.add_argument("--seeds", action="store_true",
                    help="add per-query entry rows (DESIGN.md 4ae): search_graph(seeds=16 / 32) over seed tables of 1,024 and "
                         "4,096 rows, and HZ_K_GRAPH_SEED's own time at Q = 1 and 1,024")
    ap.add_argument("--corpora", default="isotropic,clustered")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    out = open(a.out, "w")

    def emit(**kv):
        print(json.dumps(kv), flush=True)
        out.write(json.dumps(kv) + "\n")
        out.flush()

    with tempfile.TemporaryDirectory() as d:
        for kind in a.corpora.split(","):
            rows, q = corpus(kind, a.n, a.dim, 1024, rng)
            plain, graph, ivf = (os.path.join(d, f"{kind}-{x}.hzidx") for x in ("plain", "graph", "ivf"))
            S.write_index(plain, rows, "cosine")
            t = time.perf_counter()
            S.convert_index(plain, graph, "bf16", graph=a.deg, graph_backend="gpu")
            t_graph = time.perf_counter() - t
            t = time.perf_counter()
            S.convert_index(plain, ivf, "bf16", ivf=a.nlist, ivf_backend="gpu")
            t_ivf = time.perf_counter() - t
            emit(corpus=kind, n=a.n, dim=a.dim, build_graph_s=round(t_graph, 2), build_ivf_s=round(t_ivf, 2), deg=a.deg, nlist=a.nlist)
            if a.prune:
                pruned = os.path.join(d, f"{kind}-pruned.hzidx")
                t = time.perf_counter()
                S.convert_index(plain, pruned, "bf16", graph=a.deg, graph_backend="gpu", graph_prune=True)
                emit(corpus=kind, n=a.n, dim=a.dim, deg=a.deg, build_graph_s=round(t_graph, 2),
                     build_pruned_graph_s=round(time.perf_counter() - t, 2))
            tq = q[:a.truth_queries]
            truth = S.search_ref(S.bf16_to_f32(S.read_rows(plain)), tq, 10)[1]
            del rows
            with S.Index(plain) as px, S.Index(graph) as gx, S.Index(ivf) as vx, \
                    (S.Index(pruned) if a.prune else contextlib.nullcontext()) as rx, contextlib.ExitStack() as seeded:
                tables = {}
                for table in (1024, 4096) if a.seeds else ():
                    tables[table] = seeded.enter_context(S.Index(graph))
                    tables[table].set_graph(tables[table].graph, seeds=table)
                    for nq in (1, 1024):
                        for E in (16, 32):
                            emit(corpus=kind, n=a.n, kernel="HZ_K_GRAPH_SEED", S=table, E=E, Q=nq,
                                 ms=round(seed_kernel_ms(tables[table], q[:nq], E), 4))
                for w in (64, 128) if a.prune else ():
                    emit(corpus=kind, n=a.n, kernel="HZ_K_GRAPH_PRUNE", W=w, ms=round(prune_kernel_ms(px.knn_graph(w)[0]), 3))
                routes = {"search (plain scan)": lambda x: px.search(x, 10)}
                for beam, width in ((32, 1), (64, 1), (64, 2), (128, 2), (256, 4)):
                    routes[f"search_graph beam={beam} width={width}"] = lambda x, b=beam, w=width: gx.search_graph(x, 10, beam=b, width=w)
                    if a.prune:
                        routes[f"search_graph pruned beam={beam} width={width}"] = \
                            lambda x, b=beam, w=width: rx.search_graph(x, 10, beam=b, width=w)
                for table, sx in tables.items():
                    for E in (16, 32):
                        for beam, width in ((64, 1), (128, 2)):
                            routes[f"search_graph seeds={E} of {table} beam={beam} width={width}"] = \
                                lambda x, s=sx, e=E, b=beam, w=width: s.search_graph(x, 10, beam=b, width=w, seeds=e)
                for nprobe in (1, 2, 4, 8, 16, 32, 64):
                    routes[f"ivf nprobe={nprobe}"] = lambda x, p=nprobe: vx.search(x, 10, nprobe=p)
                rec = {name: recall(f(tq)[1], truth) for name, f in routes.items()}
                stats = gx.search_graph(tq, 10, beam=64, width=1, stats=True)[2]
                emit(corpus=kind, rows_scored_beam64=float(stats[:, 1].mean()), iterations_beam64=float(stats[:, 0].mean()))
                if a.prune:
                    stats = rx.search_graph(tq, 10, beam=64, width=1, stats=True)[2]
                    emit(corpus=kind, graph="pruned", rows_scored_beam64=float(stats[:, 1].mean()),
                         iterations_beam64=float(stats[:, 0].mean()))
                for nq in (1, 16, 1024):
                    part, ms = q[:nq], {name: [] for name in routes}
                    for f in routes.values():
                        f(part)  # capture
                    for _ in range(a.reps):  # interleaved: every route once per round
                        for name, f in routes.items():
                            t = time.perf_counter()
                            f(part)
                            ms[name].append((time.perf_counter() - t) * 1e3)
                    for name in routes:
                        emit(corpus=kind, Q=nq, route=name, ms=round(float(np.median(ms[name])), 3), recall_at_10=round(rec[name], 4))


if __name__ == "__main__":
    main()
