"""Time of an IVF build (``write_index(ivf=NLIST)``, what ``hipzap index --ivf NLIST`` runs) by ``ivf_backend``, and
recall@10 of the resulting index at its default nprobe (profiles/search_cluster/README.md).

    python scripts/bench_cluster.py --n 100000 --nlist 256 1024 --rounds 3 --out profiles/search_cluster/measure.jsonl

Per (N, nlist) the two backends are built in interleaved rounds (cpu, gpu, cpu, gpu, ...) on one box and the medians
are reported; the first GPU build of a process pays the code load and is reported apart (``gpu_first_s``). The vectors
are a mixture of ``4 * nlist`` Gaussian bumps in D dimensions, so that lists mean something; recall is against the
exact top 10 of a plain index of the same vectors over ``--queries`` held-out draws of the mixture. ``--parts`` also
times the two kernels of one k-means iteration through ``Index``'s hooks."""
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


def mixture(n, d, bumps, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((bumps, d)).astype(np.float32)
    out = np.empty((n, d), np.float32)
    for a in range(0, n, 1 << 16):
        lab = rng.integers(0, bumps, min(1 << 16, n - a))
        out[a:a + lab.size] = centres[lab] + np.float32(0.7) * rng.standard_normal((lab.size, d), np.float32)
    return out


def recall_at_10(path, plain, q):
    with S.Index(path) as ix, S.Index(plain) as px:
        got = ix.search(q, 10)[1]
        want = px.search(q, 10)[1]
    return float(np.mean([len(set(g) & set(w)) / 10 for g, w in zip(got.tolist(), want.tolist())]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--backends", nargs="+", default=["cpu", "gpu"])
    ap.add_argument("--parts", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="bench-cluster-")
    first_gpu = True
    for n in a.n:
        for nlist in a.nlist:
            vec = mixture(n + a.queries, a.d, 4 * nlist, 7)
            vec, q = vec[:n], vec[n:]
            plain = os.path.join(tmp, "plain.hzidx")
            S.write_index(plain, vec, "cosine")
            times = {b: [] for b in a.backends}
            rec = {"n": n, "d": a.d, "nlist": nlist, "rounds": a.rounds, "iters": 10}
            for r in range(a.rounds):
                for b in a.backends:
                    path = os.path.join(tmp, f"{b}.hzidx")
                    t0 = time.perf_counter()
                    S.write_index(path, vec, "cosine", ivf=nlist, ivf_backend=b)
                    dt = time.perf_counter() - t0
                    if b == "gpu" and first_gpu:
                        first_gpu, rec["gpu_first_s"] = False, round(dt, 3)
                        t0 = time.perf_counter()
                        S.write_index(path, vec, "cosine", ivf=nlist, ivf_backend=b)
                        dt = time.perf_counter() - t0
                    times[b].append(dt)
                    print(f"# n={n} nlist={nlist} round {r} {b}: {dt:.3f} s", flush=True)
            for b in a.backends:
                rec[f"{b}_s"] = round(statistics.median(times[b]), 3)
                rec[f"{b}_all_s"] = [round(t, 3) for t in times[b]]
                rec[f"{b}_recall10"] = round(recall_at_10(os.path.join(tmp, f"{b}.hzidx"), plain, q), 4)
            if a.parts:
                with S.Index(plain, contexts=1) as ix:
                    bits, assign, _ = ix.cluster(nlist, iters=1)
                    take = np.ones(n, bool)
                    for name, call in (("assign_all_rows_s", lambda: ix._cluster_assign(bits, take)),):
                        call()
                        ts = []
                        for _ in range(5):
                            t0 = time.perf_counter()
                            call()
                            ts.append(time.perf_counter() - t0)
                        rec[name] = round(statistics.median(ts), 4)
                    order = np.argsort(assign, kind="stable").astype(np.int32)
                    seg = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]).astype(np.int32)
                    ix._cluster_update(order, seg, bits)
                    ts = []
                    for _ in range(5):
                        t0 = time.perf_counter()
                        ix._cluster_update(order, seg, bits)
                        ts.append(time.perf_counter() - t0)
                    rec["cmean_all_rows_s"] = round(statistics.median(ts), 4)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            for name in os.listdir(tmp):
                os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
