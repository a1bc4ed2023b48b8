#!/usr/bin/env python3
"""The measurements of DESIGN.md 4ab on one MI355X; writes profiles/search_ivf_batch/search_ivf_batch.json and README.md.

D = 768, k = 10, nlist = 1024, cosine, a clustered corpus (1,000 centres, sigma 0.05 per column; the queries are corpus
rows plus a tenth of that noise), every row live. Per N in {1e5, 1e6}, Q in {64, 1024} and nprobe in {1, 16, 64}, three
routes over the SAME vectors, interleaved round by round, each a host clock around calls that end in a device
synchronise (launch to launch: H2D of the queries to D2H of the answer), medians over ``--rounds``:

  ivf_batch   ``Index.search_batch_ivf(q, 10, nprobe=p)``: the new route, fallback included
  search16    ``Index.search(q[a:a + 16], 10, nprobe=p)`` for every part of 16: the parent commit's only route
  flat_batch  ``Index.search_batch(q, 10)`` on a plain bf16 index of the same rows (no lists; once per N and Q)

The new route is also split: ``coarse`` = ``probes_batch`` alone, ``list`` = the native list call with those probes
(H2D, the inversion, three kernels, D2H), ``invert`` = the host inversion inside it (the library's own clock), and
``certified`` = the share of queries whose certificate held before the fallback.

The lists come from ``write_index(ivf_backend="gpu")``: the project's own clustering kernels, ``--iters`` rounds.

    python scripts/search_ivf_batch_measure.py [--out profiles/search_ivf_batch] [--rounds 5] [--sizes 100000,1000000] [--iters 3]"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402

D, K, NLIST = 768, 10, 1024
QS, PROBES = (64, 1024), (1, 16, 64)


def _opt(flag, default, cast=int):
    return cast(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def corpus(n, nq, seed=0, centres=1000, sigma=0.05):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, D)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    v = np.empty((n, D), np.float32)
    for a in range(0, n, 65536):
        m = min(65536, n - a)
        v[a:a + m] = c[rng.integers(0, centres, m)] + np.float32(sigma) * rng.standard_normal((m, D)).astype(np.float32)
    q = v[rng.choice(n, nq, replace=False)] + np.float32(sigma / 10) * rng.standard_normal((nq, D)).astype(np.float32)
    return v, np.ascontiguousarray(q, np.float32)


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e6, out


def measure(n, rounds, iters, work):
    rows = []
    v, qall = corpus(n, max(QS))
    ivf, flat = os.path.join(work, f"ivf{n}.hzidx"), os.path.join(work, f"flat{n}.hzidx")
    t0 = time.perf_counter()
    S.write_index(flat, v, "cosine")
    S.write_index(ivf, v, "cosine", ivf=NLIST, nprobe=16, ivf_iters=iters, ivf_backend="gpu")
    del v
    print(f"N={n}: files written in {time.perf_counter() - t0:.0f} s", flush=True)
    with S.Index(ivf, contexts=1) as ix, S.Index(flat, contexts=1) as fx:
        tiles = np.diff(S.read_ivf(ivf)["list_off"])
        for nq in QS:
            q = qall[:nq]
            parts = [q[a:a + 16] for a in range(0, nq, 16)]
            fx.search_batch(q, K)  # warm: program capture, scratch
            tf = []
            for p in PROBES:
                routes = {
                    "ivf_batch": lambda: ix.search_batch_ivf(q, K, nprobe=p),
                    "search16": lambda: [ix.search(part, K, nprobe=p) for part in parts],
                    "flat_batch": lambda: fx.search_batch(q, K),
                    "coarse": lambda: ix.probes_batch(q, p),
                }
                for fn in routes.values():  # warm every shape the timed window uses
                    fn()
                probes = ix.probes_batch(q, p)[0]
                R = S.batch_candidates(K)
                out = (np.empty((nq, K), np.float32), np.empty((nq, K), np.int32), np.empty(nq, np.float32))

                def native():
                    rc = ix._lib.hz_index_search_batch_ivf(ix._h, 0, q.ctypes.data, nq, probes.ctypes.data, p, K, R,
                                                           *(o.ctypes.data for o in out))
                    assert rc == 0, rc
                routes["list"] = native
                native()
                t = {name: [] for name in routes}
                inv = []
                for _ in range(rounds):  # interleaved: one call of every route per round
                    for name, fn in routes.items():
                        if name == "flat_batch" and tf:
                            continue
                        t[name].append(clock(fn)[0])
                    inv.append(float(ix._lib.hz_index_search_batch_ivf_invert_us(ix._h, 0)))
                tf = tf or t["flat_batch"]
                got = ix.search_batch_ivf(q, K, nprobe=p, fallback=False)
                want = np.concatenate([ix.search(part, K, nprobe=p)[1] for part in parts])
                full = ix.search_batch_ivf(q, K, nprobe=p)
                assert np.array_equal(full[1], want) and full[2].all()  # the answer is the parent route's
                med = {name: statistics.median(x) for name, x in t.items() if x}
                row = {"N": n, "Q": nq, "nprobe": p, "rounds": rounds, **{f"{k}_us": round(x, 1) for k, x in med.items()},
                       "flat_batch_us": round(statistics.median(tf), 1), "invert_us": round(statistics.median(inv), 1),
                       "certified": float(got[2].mean()), "speedup_vs_search16": round(med["search16"] / med["ivf_batch"], 2),
                       "tiles_per_list_mean": float(tiles.mean()), "spread_ivf_batch_us": [round(min(t["ivf_batch"]), 1), round(max(t["ivf_batch"]), 1)]}
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.remove(ivf), os.remove(flat)
    return rows


def main():
    out = _opt("--out", "profiles/search_ivf_batch", str)
    rounds, iters = _opt("--rounds", 5), _opt("--iters", 3)
    sizes = [int(x) for x in _opt("--sizes", "100000,1000000", str).split(",")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this script measures on a GPU and found none")
    os.makedirs(out, exist_ok=True)
    rows = []
    with tempfile.TemporaryDirectory() as work:
        for n in sizes:
            rows += measure(n, rounds, iters, work)
    name = "search_ivf_batch" + ("" if len(sizes) > 1 else f"_{sizes[0]}")
    with open(os.path.join(out, name + ".json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "D": D, "k": K, "nlist": NLIST, "rows": rows}, f, indent=1)
    head = "| N | Q | nprobe | ivf_batch us | search16 us | x | flat_batch us | coarse us | list us | invert us | certified |\n|" + "---|" * 11
    lines = [f"| {r['N']} | {r['Q']} | {r['nprobe']} | {r['ivf_batch_us']} | {r['search16_us']} | {r['speedup_vs_search16']} | "
             f"{r['flat_batch_us']} | {r['coarse_us']} | {r['list_us']} | {r['invert_us']} | {r['certified']:.3f} |" for r in rows]
    with open(os.path.join(out, name + ".md"), "w") as f:
        f.write(f"# Bulk search over IVF indexes ({torch.cuda.get_device_name(0)})\n\n{__doc__.split('    python')[0]}\n{head}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
