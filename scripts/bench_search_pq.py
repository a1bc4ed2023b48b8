#!/usr/bin/env python3
"""The measurements of profiles/search_pq/README.md on one MI355X; writes that file and search_pq.json.

D = 768, k = 10, M in {96, 48}. Every comparison is interleaved round by round in one process on one box, launch to
launch (device events around ``--launches`` back-to-back launch sequences), all rows live, no filter.

1. Time, N in {1e5, 1e6} x Q in {1, 16}: bf16 fscan + merge, fp8 qscan + merge and the binary scan + merge (the parent
   commit's kernels, re-measured here), then per M the table launch alone, the PQ scan alone, table + scan + merge at
   k = 10 and k = 128, and the two-stage sequence table + scan + merge at k = R, rescore, for R in {40, 128} with the
   bf16 rows in device memory and in pinned host memory. The codes of the timing runs are uniform random bytes over a
   random codebook: a scan's time depends on the codes only through the LDS banks they hit, and uniform codes are what
   an isotropic corpus gives; no 1e6-row corpus is trained or encoded.
2. Recall@10 and recall@1 against fp64 truth over the unquantised vectors for PQ alone and two-stage at R in
   {20, 40, 128}, beside bf16, fp8 and binary on the same rows: 4n's two corpora (1e5 x 768 cosine rows, isotropic /
   1,000 clusters sigma 0.1, 1,000 queries). Codebooks: ``pq_train`` with its defaults (10 iterations, 65,536 rows);
   the host seconds of training and encoding are recorded (``--cache DIR`` keeps codebooks and codes between runs).
3. Device bytes of an open index per placement (``Index.describe()``), beside the bf16, fp8 and binary indexes.
4. ``--span-sweep``: the scan alone at N = 1e6 for every M bucket, Q in {1, 4, 16} and span in 1 .. 128 beside the
   launcher's choice (span.json; what ``pq_auto_span`` in csrc/search.hip was fitted to).

    python scripts/bench_search_pq.py [--out profiles/search_pq] [--rounds 7] [--launches 50] [--sizes 100000,1000000]"""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hipzap import _native as NV  # noqa: E402
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

from bench_search_bin import Runs, sign_words  # noqa: E402
from search_fp8_measure import DEV, D, K, _dev_u32, _opt, _time, device_corpora  # noqa: E402

MS = (96, 48)
RS = (40, 128)


class PqRuns:
    """The PQ launches over one code block [N, M] for the queries, buffers and rescore rows of a ``Runs``."""

    def __init__(self, L, codes, cb):
        self.L, self.codes, self.cb, self.M = L, codes, cb, codes.shape[1]
        self.lut = torch.zeros(L.Q, self.M, 256, device=DEV)
        self.lp = OS.PqLutParams(L.q.data_ptr(), cb.data_ptr(), self.lut.data_ptr(), self.lut.numel() * 4, D, self.M, L.Q, 0)

    def _scan(self, k, out_sc, out_id, span=0):
        L = self.L
        return L._block(OS.PqScanParams, self.codes, k, out_sc, out_id, self.M, None, self.lut.data_ptr(), self.lut.numel() * 4,
                        self.M, span)

    def lut_alone(self):
        return lambda: (OS.launch_pq_lut(self.lp, self.L.st), 0)

    def scan_alone(self, k, span=0):
        p, lib = self._scan(k, self.L.sc, self.L.ids, span), NV.lib()
        return lambda: (lib.hz_search_pqscan_launch(C.byref(p), self.L.st), 0)

    def search(self, k, out=None):
        p = self._scan(k, *(out or (self.L.sc, self.L.ids)))

        def run():
            rc = OS.launch_pq_lut(self.lp, self.L.st)
            rs = OS.launch_pq(p, self.L.st)
            return (rc or rs[0], rs[1])
        return run

    def two_stage(self, R, place, k=K):
        L = self.L
        one = self.search(R, (L.msc, L.mid))
        p2 = OS.RescoreParams(L.rows[place], L.q.data_ptr(), L.mid.data_ptr(), L.sc.data_ptr(), L.ids.data_ptr(), L.N, D, L.Q, R,
                              k, D)
        return lambda: (one(), OS.launch_rescore(p2, L.st))


def speed(N, rounds, launches):
    bf, codes, scales = device_corpora(N, N)
    words = sign_words(bf)
    host = torch.empty(N, D, dtype=torch.bfloat16, pin_memory=True)
    host.copy_(bf)
    g = torch.Generator(device=DEV).manual_seed(N + 1)
    pq = {M: (torch.randint(0, 256, (N, M), generator=g, device=DEV, dtype=torch.uint8),
              torch.randn(M, 256, D // M, generator=g, device=DEV) * (D ** -0.5)) for M in MS}
    out = []
    for Q in (1, 16):
        q = torch.randn(Q, D, generator=g, device=DEV)
        q = q / q.norm(dim=1, keepdim=True)
        L = Runs(bf, codes, scales, words, q, host)
        runs = {"bf16 fscan+merge k=10": L.bf16(K), "fp8 qscan+merge k=10": L.fp8(K), "bin scan+merge k=10": L.bin(K),
                "bin scan+merge k=128": L.bin(128), "bin two-stage R=40 device": L.two_stage(40, "device"),
                "bin two-stage R=128 device": L.two_stage(128, "device")}
        spans = {}
        for M in MS:
            P = PqRuns(L, *pq[M])
            spans[f"M={M}"] = OS.pq_span(N, Q, M)
            runs[f"pq M={M} table alone"] = P.lut_alone()
            runs[f"pq M={M} scan alone k=10"] = P.scan_alone(K)
            runs[f"pq M={M} scan alone k=10, span=1"] = P.scan_alone(K, 1)
            runs[f"pq M={M} table+scan+merge k=10"] = P.search(K)
            runs[f"pq M={M} table+scan+merge k=128"] = P.search(128)
            for R in RS:
                for place in ("device", "host"):
                    runs[f"pq M={M} two-stage R={R} {place}"] = P.two_stage(R, place)
        us = {n: [] for n in runs}
        for fn in runs.values():  # every refusal shows here, before anything is timed
            rc = fn()
            assert rc in ((0, 0), ((0, 0), 0)), rc
        torch.cuda.synchronize()
        for _ in range(rounds):
            for n, fn in runs.items():
                us[n].append(_time(fn, launches))
        out.append({"N": N, "Q": Q, "rounds": rounds, "launches_per_round": launches, "auto_span": spans,
                    "us_median": {n: round(statistics.median(v), 1) for n, v in us.items()},
                    "us_spread": {n: round(max(v) - min(v), 1) for n, v in us.items()},
                    "row_bytes": {"bf16": N * D * 2, "fp8": N * D + N * 4, "bin": N * D // 8, **{f"pq M={M}": N * M for M in MS}}})
        print(json.dumps(out[-1]), flush=True)
    return out


def span_sweep(N=1000000, rounds=3, launches=20):
    bf, codes, scales = device_corpora(N, N)
    words = sign_words(bf)
    g = torch.Generator(device=DEV).manual_seed(5)
    out = {}
    for M in (96, 64, 48, 32, 16):  # the buckets that divide 768
        pq = (torch.randint(0, 256, (N, M), generator=g, device=DEV, dtype=torch.uint8),
              torch.randn(M, 256, D // M, generator=g, device=DEV) * (D ** -0.5))
        for Q in (1, 4, 16):
            L = Runs(bf, codes, scales, words, torch.randn(Q, D, generator=g, device=DEV), None)
            P = PqRuns(L, *pq)
            assert P.lut_alone()() == (0, 0)
            runs = {s: P.scan_alone(K, s) for s in (1, 2, 4, 8, 16, 32, 64, 128, 0)}
            us = {s: [] for s in runs}
            for _ in range(rounds):
                for s, fn in runs.items():
                    us[s].append(_time(fn, launches))
            out[f"M={M} Q={Q}"] = {f"auto={OS.pq_span(N, Q, M)}" if s == 0 else str(s): round(statistics.median(v), 1)
                                   for s, v in us.items()}
            print(f"M={M} Q={Q}", json.dumps(out[f"M={M} Q={Q}"]), flush=True)
    return out


def trained(name, M, rows32, cache):
    """(codes, codebook, host seconds of training, of encoding); kept in ``cache`` when given."""
    path = os.path.join(cache, f"pq_{name}_m{M}.npz") if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return z["codes"], z["codebook"], float(z["train_s"]), float(z["encode_s"])
    t0 = time.time()
    cb = S.pq_train(rows32, M)
    t1 = time.time()
    codes = S.pq_encode(rows32, cb)
    t2 = time.time()
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez(path, codes=codes, codebook=cb, train_s=t1 - t0, encode_s=t2 - t1)
    return codes, cb, t1 - t0, t2 - t1


def corpus(name, N=100000, NQ=1000, seed=7):
    rng = np.random.default_rng(seed)
    if name == "isotropic":
        return rng.standard_normal((N, D), dtype=np.float32), rng.standard_normal((NQ, D), dtype=np.float32)
    centres = rng.standard_normal((1000, D), dtype=np.float32)
    v = centres[rng.integers(0, 1000, N)] + np.float32(0.1) * rng.standard_normal((N, D), dtype=np.float32)
    return v, centres[rng.integers(0, 1000, NQ)] + np.float32(0.1) * rng.standard_normal((NQ, D), dtype=np.float32)


def quality(name, cache, keep=None):
    v, q = corpus(name)
    N, NQ = v.shape[0], q.shape[0]
    if keep is not None:
        keep.append(v)
    vn, qn = S.normalize_rows(v), S.normalize_rows(q)
    truth = torch.from_numpy(qn).to(DEV).double() @ torch.from_numpy(vn).to(DEV).double().T  # fp64 [NQ, N]
    tid = truth.topk(K, dim=1).indices.cpu().numpy()
    del truth
    bits = S.prepare_rows(v, "cosine")
    codes, scales = S.prepare_rows_fp8(v, "cosine")
    words = S.prepare_rows_bin(v, "cosine")
    bf = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.bfloat16)
    cd, sd, wd = torch.from_numpy(codes).to(DEV), torch.from_numpy(scales).to(DEV), _dev_u32(words)
    host = {}
    pq = {}
    for M in MS:
        c, cb, ts, es = trained(name, M, S.bf16_to_f32(bits), cache)
        host[f"M={M}"] = {"train_s": round(ts, 1), "encode_s": round(es, 1),
                          "distortion": round(S.pq_distortion(S.bf16_to_f32(bits[:10000]), cb), 5)}
        pq[M] = (torch.from_numpy(c).to(DEV), torch.from_numpy(cb).to(DEV))
        print(json.dumps({"corpus": name, "M": M, **host[f"M={M}"]}), flush=True)
    names = ["bf16", "fp8", "bin alone", "bin two-stage R=128"]
    for M in MS:
        names += [f"pq M={M} alone"] + [f"pq M={M} two-stage R={R}" for R in (20, 40, 128)]
    got = {n: [] for n in names}
    for a in range(0, NQ, 16):
        L = Runs(bf, cd, sd, wd, torch.from_numpy(qn[a:a + 16]).to(DEV))
        got["bf16"].append(L.result(L.bf16(K)))
        got["fp8"].append(L.result(L.fp8(K)))
        got["bin alone"].append(L.result(L.bin(K)))
        got["bin two-stage R=128"].append(L.result(L.two_stage(128, "device")))
        for M in MS:
            P = PqRuns(L, *pq[M])
            got[f"pq M={M} alone"].append(L.result(P.search(K)))
            for R in (20, 40, 128):
                got[f"pq M={M} two-stage R={R}"].append(L.result(P.two_stage(R, "device")))
    out = {"corpus": name, "N": N, "queries": NQ, "k": K, "host": host}
    for n, parts in got.items():
        ids = np.concatenate(parts)
        out[n] = {"recall_at_10": round(float(np.mean([len(set(a) & set(b)) / K for a, b in zip(ids, tid)])), 4),
                  "recall_at_1": round(float(np.mean(ids[:, 0] == tid[:, 0])), 4)}
    print(json.dumps(out), flush=True)
    return out


def device_bytes(v, cache):
    out = {}
    bits = S.prepare_rows(v, "cosine")
    with tempfile.TemporaryDirectory() as tmp:
        p = {n: os.path.join(tmp, n + ".hzidx") for n in ("v1", "v3", "v8", "v10_96", "v10_48", "v11_96")}
        S.write_index(p["v1"], v)
        S.write_index(p["v3"], v, dtype="fp8")
        S.write_index(p["v8"], v, dtype="bin")
        cbs = {M: trained("isotropic", M, S.bf16_to_f32(bits), cache)[1] for M in MS}
        S.write_index(p["v10_96"], v, dtype="pq", pq_m=96, pq_codebook=cbs[96])
        S.write_index(p["v10_48"], v, dtype="pq", pq_m=48, pq_codebook=cbs[48])
        S.write_index(p["v11_96"], v, dtype="pq", pq_m=96, pq_codebook=cbs[96], rescore=True)
        for name, path, kw in (("bf16 index", p["v1"], {}), ("fp8 index", p["v3"], {}), ("binary index", p["v8"], {}),
                               ("pq index M=96", p["v10_96"], {}), ("pq index M=48", p["v10_48"], {}),
                               ("pq M=96 two-stage, rows on the device", p["v11_96"], {"rescore_rows": "device"}),
                               ("pq M=96 two-stage, rows in pinned host memory", p["v11_96"], {"rescore_rows": "host"})):
            with S.Index(path, **kw) as ix:
                d = ix.describe()
                out[name] = d["device_bytes"]
                if "scan_span" in d:
                    out[name + ": codebook bytes"] = d["codebook_bytes"]
    print(json.dumps(out), flush=True)
    return out


def main():
    out_dir = _opt("--out", "profiles/search_pq", str)
    cache = _opt("--cache", "", str)
    rounds, launches = _opt("--rounds", 7), _opt("--launches", 50)
    sizes = [int(x) for x in _opt("--sizes", "100000,1000000", str).split(",")]
    os.makedirs(out_dir, exist_ok=True)
    if "--span-sweep" in sys.argv:
        with open(os.path.join(out_dir, "span.json"), "w") as f:
            json.dump({"N": 1000000, "D": D, "k": K, "us_median_scan_alone": span_sweep()}, f, indent=1)
        return
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tile_rows": OS.tile_rows(), "D": D, "k": K,
           "speed": [], "quality": []}
    for N in sizes:
        res["speed"] += speed(N, rounds, launches)
    keep = []
    for name in ("isotropic", "clusters"):
        res["quality"].append(quality(name, cache, keep=keep if name == "isotropic" else None))
    res["device_bytes"] = device_bytes(keep[0], cache)
    with open(os.path.join(out_dir, "search_pq.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Product-quantised vector indexes: table + ADC scan, exact bf16 rescoring (scripts/bench_search_pq.py)", "",
             f"Device: {res['device']}, torch {res['torch']}. D = {D}, k = {K}, tile = {res['tile_rows']} rows. Raw: search_pq.json.", "",
             "## Time, launch to launch", "",
             f"Device events around {launches} back-to-back launch sequences; medians (us) over {rounds} rounds, every variant "
             "interleaved within each round; in brackets the spread (max - min) over the rounds. All rows live, no filter. The "
             "bf16, fp8 and binary rows are the existing kernels re-measured in the same rounds. `two-stage` = table + scan + "
             "merge at k = R, then the rescore launch at k = 10; `device` / `host` is where the bf16 rows lie. The PQ codes of "
             "these runs are uniform random bytes. `auto span` (tiles per workgroup): "
             + "; ".join(f"N = {c['N']}, Q = {c['Q']}: {c['auto_span']['M=96']} (M = 96), {c['auto_span']['M=48']} (M = 48)"
                         for c in res["speed"]) + ".", ""]
    names = list(res["speed"][0]["us_median"])
    lines += ["| variant | " + " | ".join(f"N = {c['N']}, Q = {c['Q']}" for c in res["speed"]) + " |",
              "|---|" + "---|" * len(res["speed"])]
    for n in names:
        lines.append(f"| {n} | " + " | ".join(f"{c['us_median'][n]} [{c['us_spread'][n]}]" for c in res["speed"]) + " |")
    lines += ["", "## Recall against fp64 truth over the unquantised vectors", "",
              "1e5 x 768 cosine rows, 1,000 queries drawn like the rows. `clusters`: 1,000 centres N(0, I), rows = centre + "
              "0.1 * N(0, I). recall@10 / recall@1.", ""]
    cols = [n for n in res["quality"][0] if n not in ("corpus", "N", "queries", "k", "host")]
    lines += ["| variant | " + " | ".join(c["corpus"] for c in res["quality"]) + " |", "|---|" + "---|" * len(res["quality"])]
    for n in cols:
        lines.append(f"| {n} | " + " | ".join(f"{c[n]['recall_at_10']} / {c[n]['recall_at_1']}" for c in res["quality"]) + " |")
    lines += ["", "## Host cost of a codebook and of encoding 1e5 rows (numpy, seconds; mean squared error per row)", "",
              "| corpus | M | train | encode | distortion |", "|---|---|---|---|---|"]
    for c in res["quality"]:
        for m, h in c["host"].items():
            lines.append(f"| {c['corpus']} | {m[2:]} | {h['train_s']} | {h['encode_s']} | {h['distortion']} |")
    lines += ["", "## Device bytes of an open index (1e5 x 768, two contexts)", "", "| index | device bytes |", "|---|---|"]
    lines += [f"| {n} | {b} |" for n, b in res["device_bytes"].items()]
    lines.append("")
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
