#!/usr/bin/env python3
"""The measurements of profiles/search_bin/README.md on one MI355X; writes that file and search_bin.json.

D = 768, k = 10. Every comparison is interleaved round by round in one process on one box, launch to launch (device
events around ``--launches`` back-to-back launch sequences), all rows live, no filter.

1. Time, N in {1e5, 1e6} x Q in {1, 16}: bf16 fscan + merge, fp8 qscan + merge, the binary scan + merge at k = 10
   and k = 128, and the two-stage sequence binary scan + merge at k = R, rescore, for R in {40, 128} with the bf16 rows
   in device memory and in pinned host memory.
2. How the binary scan's time splits: the scan launch alone over the live corpus (staging, loads, scoring, ranking)
   and over the same corpus with an all-zero live bitmap, where no row is loaded or scored and every thread still
   walks the ranking loop (staging and ranking); the difference is loading and scoring.
3. Recall@10 and recall@1 against fp64 truth over the unquantised vectors for the sign bits alone and two-stage at
   R in {20, 40, 128}: 4n's two corpora (1e5 x 768 cosine rows, isotropic / 1,000 clusters sigma 0.1, 1,000 queries).
4. Device bytes of an open index per placement (``Index.describe()``), beside the bf16 and the fp8 index.

    python scripts/bench_search_bin.py [--out profiles/search_bin] [--rounds 7] [--launches 50] [--sizes 100000,1000000]"""
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

from search_fp8_measure import DEV, D, K, _dev_u32, _opt, _time, device_corpora  # noqa: E402

W = D // 32
RS = (40, 128)


def sign_words(bf):
    """bf16 rows on the device -> their sign-bit words int32 [N, W] (bit i & 31 of word i >> 5: sign clear)."""
    out = torch.empty(bf.shape[0], W, dtype=torch.int32, device=DEV)
    weight = (torch.ones(32, dtype=torch.int64, device=DEV) << torch.arange(32, device=DEV))
    for a in range(0, bf.shape[0], 65536):
        clear = (bf[a:a + 65536].view(torch.int16) >= 0).view(-1, W, 32).to(torch.int64)
        out[a:a + 65536] = ((clear * weight).sum(dim=2) & 0xFFFFFFFF).to(torch.int32)  # wraps into the sign bit
    return out


class Runs:
    """The launches over one corpus in its three formats for a given Q."""

    def __init__(self, bf, codes, scales, words, q, host_rows=None):
        N, Q = bf.shape[0], q.shape[0]
        self.Q, self.N, self.q = Q, N, q
        self.nbytes = OS.scratch_bytes(N, Q, 128)
        self.cand = torch.zeros(self.nbytes // 8, dtype=torch.int64, device=DEV)
        self.sc, self.ids = torch.empty(Q, 128, device=DEV), torch.empty(Q, 128, dtype=torch.int32, device=DEV)
        self.msc, self.mid = torch.empty(Q, 128, device=DEV), torch.full((Q, 128), -1, dtype=torch.int32, device=DEV)
        self.live_words = S.pack_live(np.ones(N, bool))
        self.lv = _dev_u32(self.live_words)
        self.dead = torch.zeros_like(self.lv)
        self.keep = (bf, codes, scales, words, host_rows)
        self.st = torch.cuda.current_stream().cuda_stream
        self.rows = {"device": bf.data_ptr(), "host": host_rows.data_ptr() if host_rows is not None else 0}

    def _block(self, cls, corpus, k, out_sc, out_id, ldc, live=None, *more):
        return cls(corpus.data_ptr(), self.q.data_ptr(), self.cand.data_ptr(), out_sc.data_ptr(), out_id.data_ptr(), self.N, D,
                   self.Q, k, ldc, 0, self.nbytes, (self.lv if live is None else live).data_ptr(), 0, 0,
                   self.live_words.size * 4, *more)

    def bf16(self, k):
        p = self._block(OS.FilterScanParams, self.keep[0], k, self.sc, self.ids, D)
        return lambda: OS.launch_filtered(p, self.st)

    def fp8(self, k):
        p = self._block(OS.QuantScanParams, self.keep[1], k, self.sc, self.ids, D, None, self.keep[2].data_ptr())
        return lambda: OS.launch_quant(p, self.st)

    def bin(self, k):
        p = self._block(OS.BinScanParams, self.keep[3], k, self.sc, self.ids, W)
        return lambda: OS.launch_bin(p, self.st)

    def bin_scan_alone(self, k, dead=False):
        import ctypes as C
        from hipzap import _native as N
        p = self._block(OS.BinScanParams, self.keep[3], k, self.sc, self.ids, W, self.dead if dead else None)
        lib = N.lib()
        return lambda: (lib.hz_search_bscan_launch(C.byref(p), self.st), 0)

    def two_stage(self, R, place, k=K):
        p1 = self._block(OS.BinScanParams, self.keep[3], R, self.msc, self.mid, W)
        p2 = OS.RescoreParams(self.rows[place], self.q.data_ptr(), self.mid.data_ptr(), self.sc.data_ptr(), self.ids.data_ptr(),
                              self.N, D, self.Q, R, k, D)

        def run():
            rc = OS.launch_bin(p1, self.st)
            return rc, OS.launch_rescore(p2, self.st)
        return run

    def result(self, fn, k=K):
        rc = fn()
        assert rc in ((0, 0), ((0, 0), 0)), rc
        torch.cuda.synchronize()
        return self.ids.cpu().numpy().reshape(-1)[:self.Q * k].reshape(self.Q, k).copy()


def speed(N, rounds, launches):
    bf, codes, scales = device_corpora(N, N)
    words = sign_words(bf)
    host = torch.empty(N, D, dtype=torch.bfloat16, pin_memory=True)
    host.copy_(bf)
    g = torch.Generator(device=DEV).manual_seed(N + 1)
    out = []
    for Q in (1, 16):
        q = torch.randn(Q, D, generator=g, device=DEV)
        q = q / q.norm(dim=1, keepdim=True)
        L = Runs(bf, codes, scales, words, q, host)
        runs = {"bf16 fscan+merge k=10": L.bf16(K), "fp8 qscan+merge k=10": L.fp8(K), "bin scan+merge k=10": L.bin(K),
                "bin scan+merge k=128": L.bin(128)}
        for R in RS:
            for place in ("device", "host"):
                runs[f"two-stage R={R} {place}"] = L.two_stage(R, place)
        for k in (K, 128):
            runs[f"bin scan alone k={k}"] = L.bin_scan_alone(k)
            runs[f"bin scan alone k={k}, no live row (staging + ranking)"] = L.bin_scan_alone(k, dead=True)
        same = {R: bool(np.array_equal(L.result(L.two_stage(R, "device")), L.result(L.two_stage(R, "host")))) for R in RS}
        top = {"two-stage R=128 equals bf16 ids": bool(np.array_equal(L.result(L.two_stage(128, "device")), L.result(L.bf16(K))))}
        us = {n: [] for n in runs}
        for _ in range(rounds):
            for n, fn in runs.items():
                us[n].append(_time(fn, launches))
        med = {n: round(statistics.median(v), 1) for n, v in us.items()}
        split = {}
        for k in (K, 128):
            total, rank = med[f"bin scan alone k={k}"], med[f"bin scan alone k={k}, no live row (staging + ranking)"]
            split[f"k={k}"] = {"scan_us": total, "staging_and_ranking_us": rank, "loading_and_scoring_us": round(total - rank, 1)}
        out.append({"N": N, "Q": Q, "rounds": rounds, "launches_per_round": launches, "host_equals_device_ids": same, **top,
                    "us_median": med, "us_spread": {n: round(max(v) - min(v), 1) for n, v in us.items()}, "split": split,
                    "row_bytes": {"bf16": N * D * 2, "fp8": N * D + N * 4, "bin": N * W * 4}})
        print(json.dumps(out[-1]), flush=True)
    return out


def quality(name, N=100000, NQ=1000, seed=7, keep=None):
    rng = np.random.default_rng(seed)
    if name == "isotropic":
        v, q = rng.standard_normal((N, D), dtype=np.float32), rng.standard_normal((NQ, D), dtype=np.float32)
    else:
        centres = rng.standard_normal((1000, D), dtype=np.float32)
        v = centres[rng.integers(0, 1000, N)] + np.float32(0.1) * rng.standard_normal((N, D), dtype=np.float32)
        q = centres[rng.integers(0, 1000, NQ)] + np.float32(0.1) * rng.standard_normal((NQ, D), dtype=np.float32)
    if keep is not None:
        keep.append(v)
    vn, qn = S.normalize_rows(v), S.normalize_rows(q)
    truth = torch.from_numpy(qn).to(DEV).double() @ torch.from_numpy(vn).to(DEV).double().T  # fp64 [NQ, N]
    tid = truth.topk(K, dim=1).indices.cpu().numpy()
    bits = S.prepare_rows(v, "cosine")
    codes, scales = S.prepare_rows_fp8(v, "cosine")
    words = S.prepare_rows_bin(v, "cosine")
    bf = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.bfloat16)
    cd, sd, wd = torch.from_numpy(codes).to(DEV), torch.from_numpy(scales).to(DEV), _dev_u32(words)
    names = ["bf16", "fp8", "bin alone"] + [f"two-stage R={R}" for R in (20, 40, 128)]
    got = {n: [] for n in names}
    for a in range(0, NQ, 16):
        L = Runs(bf, cd, sd, wd, torch.from_numpy(qn[a:a + 16]).to(DEV))
        got["bf16"].append(L.result(L.bf16(K)))
        got["fp8"].append(L.result(L.fp8(K)))
        got["bin alone"].append(L.result(L.bin(K)))
        for R in (20, 40, 128):
            got[f"two-stage R={R}"].append(L.result(L.two_stage(R, "device")))
    out = {"corpus": name, "N": N, "queries": NQ, "k": K}
    for n, parts in got.items():
        ids = np.concatenate(parts)
        out[n] = {"recall_at_10": round(float(np.mean([len(set(a) & set(b)) / K for a, b in zip(ids, tid)])), 4),
                  "recall_at_1": round(float(np.mean(ids[:, 0] == tid[:, 0])), 4)}
    print(json.dumps(out), flush=True)
    return out


def device_bytes(v):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        p9, p8, p3, p1 = (os.path.join(tmp, n) for n in ("v9.hzidx", "v8.hzidx", "v3.hzidx", "v1.hzidx"))
        S.write_index(p9, v, dtype="bin", rescore=True)
        S.write_index(p8, v, dtype="bin")
        S.write_index(p3, v, dtype="fp8")
        S.write_index(p1, v)
        for name, path, kw in (("bf16 index", p1, {}), ("fp8 index", p3, {}), ("binary index", p8, {}),
                               ("binary two-stage, rows on the device", p9, {"rescore_rows": "device"}),
                               ("binary two-stage, rows in pinned host memory", p9, {"rescore_rows": "host"})):
            with S.Index(path, **kw) as ix:
                out[name] = ix.describe()["device_bytes"]
    print(json.dumps(out), flush=True)
    return out


def main():
    out_dir = _opt("--out", "profiles/search_bin", str)
    rounds, launches = _opt("--rounds", 7), _opt("--launches", 50)
    sizes = [int(x) for x in _opt("--sizes", "100000,1000000", str).split(",")]
    os.makedirs(out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tile_rows": OS.tile_rows(), "D": D, "k": K,
           "speed": [], "quality": []}
    for N in sizes:
        res["speed"] += speed(N, rounds, launches)
    keep = []
    for name in ("isotropic", "clusters"):
        res["quality"].append(quality(name, keep=keep if name == "isotropic" else None))
    res["device_bytes"] = device_bytes(keep[0])
    with open(os.path.join(out_dir, "search_bin.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Binary vector indexes: sign-bit scan, exact bf16 rescoring of the candidates (scripts/bench_search_bin.py)", "",
             f"Device: {res['device']}, torch {res['torch']}. D = {D}, k = {K}, tile = {res['tile_rows']} rows. Raw: search_bin.json.", "",
             "## Time, launch to launch", "",
             f"Device events around {launches} back-to-back launch sequences; medians (us) over {rounds} rounds, every variant "
             "interleaved within each round; in brackets the spread (max - min) over the rounds. All rows live, no filter. "
             "`two-stage` = binary scan + merge at k = R, then the rescore launch at k = 10; `device` / `host` is where the "
             "bf16 rows lie. `scan alone` has no merge; with no live row nothing is loaded or scored and the ranking loop "
             "still runs.", ""]
    names = list(res["speed"][0]["us_median"])
    lines += ["| variant | " + " | ".join(f"N = {c['N']}, Q = {c['Q']}" for c in res["speed"]) + " |",
              "|---|" + "---|" * len(res["speed"])]
    for n in names:
        lines.append(f"| {n} | " + " | ".join(f"{c['us_median'][n]} [{c['us_spread'][n]}]" for c in res["speed"]) + " |")
    lines += ["", "## The binary scan's time: loading + scoring against staging + ranking (us, from the medians above)", "",
              "| N, Q | k | scan | staging + ranking | loading + scoring |", "|---|---|---|---|---|"]
    for c in res["speed"]:
        for k, s in c["split"].items():
            lines.append(f"| {c['N']}, {c['Q']} | {k[2:]} | {s['scan_us']} | {s['staging_and_ranking_us']} | {s['loading_and_scoring_us']} |")
    lines += ["", "## Recall against fp64 truth over the unquantised vectors", "",
              "1e5 x 768 cosine rows, 1,000 queries drawn like the rows. `clusters`: 1,000 centres N(0, I), rows = centre + "
              "0.1 * N(0, I). recall@10 / recall@1.", ""]
    cols = [n for n in res["quality"][0] if n not in ("corpus", "N", "queries", "k")]
    lines += ["| corpus | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    for c in res["quality"]:
        lines.append(f"| {c['corpus']} | " + " | ".join(f"{c[n]['recall_at_10']} / {c[n]['recall_at_1']}" for n in cols) + " |")
    lines += ["", "## Device bytes of an open index (1e5 x 768, two contexts)", "", "| index | device bytes |", "|---|---|"]
    lines += [f"| {n} | {b} |" for n, b in res["device_bytes"].items()]
    lines.append("")
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
