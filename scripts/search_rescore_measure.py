#!/usr/bin/env python3
"""The measurements of profiles/search_rescore/README.md on one MI355X; writes that file and search_rescore.json.

D = 768, k = 10. Every comparison is interleaved round by round on one box, launch to launch (device events around
``--launches`` back-to-back launch sequences), all rows live, no filter.

1. Time, N in {1e5, 1e6} x Q in {1, 16}: qscan + merge at k = 10 (the one-stage fp8 path) against the two-stage
   sequence qscan + merge at k = R, rescore, for R in {10, 40, 128} with the bf16 rows in device memory and in pinned
   host memory; bf16 fscan + merge alongside; the rescore launch alone; qscan + merge at k = 128.
2. Recall@10 and recall@1 against fp64 truth over the unquantised vectors for bf16, fp8 and two-stage at R in
   {10, 20, 40, 128}: 4n's two corpora (1e5 x 768 cosine rows, isotropic / 1,000 clusters sigma 0.1, 1,000 queries).
3. Device bytes of an open index per placement (``Index.describe()``), beside the fp8 and the bf16 index.

    python scripts/search_rescore_measure.py [--out profiles/search_rescore] [--rounds 7] [--launches 50] [--sizes 100000,1000000]"""
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

from search_fp8_measure import DEV, D, K, _dev_u32, _opt, _time, device_corpora  # noqa: E402

RS = (10, 40, 128)


class Two:
    """The launches over one pair of corpora for a given Q: one-stage (bf16, fp8 at any k) and two-stage."""

    def __init__(self, bf, codes, scales, q, host_rows=None):
        N, Q = bf.shape[0], q.shape[0]
        self.Q, self.N = Q, N
        self.nbytes = OS.scratch_bytes(N, Q, 128)
        self.cand = torch.zeros(self.nbytes // 8, dtype=torch.int64, device=DEV)
        self.sc, self.ids = torch.empty(Q, 128, device=DEV), torch.empty(Q, 128, dtype=torch.int32, device=DEV)
        self.msc, self.mid = torch.empty(Q, 128, device=DEV), torch.full((Q, 128), -1, dtype=torch.int32, device=DEV)
        self.words = S.pack_live(np.ones(N, bool))
        self.lv = _dev_u32(self.words)
        self.keep = (bf, codes, scales, q, host_rows)
        self.st = torch.cuda.current_stream().cuda_stream
        self.rows = {"device": bf.data_ptr(), "host": host_rows.data_ptr() if host_rows is not None else 0}
        self.q = q

    def _scan(self, corpus, k, out_sc, out_id, scales=None):
        tail = (self.lv.data_ptr(), 0, 0, self.words.size * 4)
        out = (self.cand.data_ptr(), out_sc.data_ptr(), out_id.data_ptr(), self.N, D, self.Q, k, D, 0, self.nbytes)
        if scales is None:
            return OS.FilterScanParams(corpus.data_ptr(), self.q.data_ptr(), *out, *tail)
        return OS.QuantScanParams(corpus.data_ptr(), self.q.data_ptr(), *out, *tail, scales.data_ptr())

    def one_stage(self, fp8, k):
        bf, codes, scales = self.keep[:3]
        p = self._scan(codes, k, self.sc, self.ids, scales) if fp8 else self._scan(bf, k, self.sc, self.ids)
        launch = OS.launch_quant if fp8 else OS.launch_filtered
        return lambda: launch(p, self.st)

    def rescore(self, R, place, k=K):
        p = OS.RescoreParams(self.rows[place], self.q.data_ptr(), self.mid.data_ptr(), self.sc.data_ptr(), self.ids.data_ptr(),
                             self.N, D, self.Q, R, k, D)
        return lambda: OS.launch_rescore(p, self.st)

    def two_stage(self, R, place, k=K):
        codes, scales = self.keep[1:3]
        p1 = self._scan(codes, R, self.msc, self.mid, scales)
        second = self.rescore(R, place, k)

        def run():
            rc = OS.launch_quant(p1, self.st)
            return rc, second()
        return run

    def result(self, fn, k=K):
        rc = fn()
        assert rc in ((0, 0), ((0, 0), 0)), rc
        torch.cuda.synchronize()
        return self.sc.cpu().numpy().reshape(-1)[:self.Q * k].reshape(self.Q, k).copy(), \
            self.ids.cpu().numpy().reshape(-1)[:self.Q * k].reshape(self.Q, k).copy()


def speed(N, rounds, launches):
    bf, codes, scales = device_corpora(N, N)
    host = torch.empty(N, D, dtype=torch.bfloat16, pin_memory=True)
    host.copy_(bf)
    g = torch.Generator(device=DEV).manual_seed(N + 1)
    out = []
    for Q in (1, 16):
        q = torch.randn(Q, D, generator=g, device=DEV)
        q = q / q.norm(dim=1, keepdim=True)
        L = Two(bf, codes, scales, q, host)
        runs = {"bf16 fscan+merge k=10": L.one_stage(False, K), "fp8 qscan+merge k=10": L.one_stage(True, K),
                "fp8 qscan+merge k=128": L.one_stage(True, 128)}
        for R in RS:
            for place in ("device", "host"):
                runs[f"two-stage R={R} {place}"] = L.two_stage(R, place)
        for R in RS:  # after a two-stage run at R = 128 the intermediate ids are real candidates
            for place in ("device", "host"):
                runs[f"rescore alone R={R} {place}"] = L.rescore(R, place)
        same = {R: bool(np.array_equal(L.result(L.two_stage(R, "device"))[1], L.result(L.two_stage(R, "host"))[1])) for R in RS}
        L.result(L.two_stage(128, "device"))
        us = {n: [] for n in runs}
        for _ in range(rounds):
            for n, fn in runs.items():
                us[n].append(_time(fn, launches))
        out.append({"N": N, "Q": Q, "rounds": rounds, "launches_per_round": launches, "host_equals_device_ids": same,
                    "us_median": {n: round(statistics.median(v), 1) for n, v in us.items()},
                    "us_spread": {n: round(max(v) - min(v), 1) for n, v in us.items()}})
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
    bf = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.bfloat16)
    cd, sd = torch.from_numpy(codes).to(DEV), torch.from_numpy(scales).to(DEV)
    names = ["bf16", "fp8"] + [f"two-stage R={R}" for R in (10, 20, 40, 128)]
    got = {n: [] for n in names}
    for a in range(0, NQ, 16):
        L = Two(bf, cd, sd, torch.from_numpy(qn[a:a + 16]).to(DEV))
        got["bf16"].append(L.result(L.one_stage(False, K))[1])
        got["fp8"].append(L.result(L.one_stage(True, K))[1])
        for R in (10, 20, 40, 128):
            got[f"two-stage R={R}"].append(L.result(L.two_stage(R, "device"))[1])
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
        p4, p3, p1 = (os.path.join(tmp, n) for n in ("v4.hzidx", "v3.hzidx", "v1.hzidx"))
        S.write_index(p4, v, dtype="fp8", rescore=True)
        S.write_index(p3, v, dtype="fp8")
        S.write_index(p1, v)
        for name, path, kw in (("bf16 index", p1, {}), ("fp8 index", p3, {}), ("two-stage, rows on the device", p4, {"rescore_rows": "device"}),
                               ("two-stage, rows in pinned host memory", p4, {"rescore_rows": "host"})):
            with S.Index(path, **kw) as ix:
                out[name] = ix.describe()["device_bytes"]
    print(json.dumps(out), flush=True)
    return out


def main():
    out_dir = _opt("--out", "profiles/search_rescore", str)
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
    with open(os.path.join(out_dir, "search_rescore.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# Two-stage search: fp8 scan, exact bf16 rescoring of the candidates (scripts/search_rescore_measure.py)", "",
             f"Device: {res['device']}, torch {res['torch']}. D = {D}, k = {K}, tile = {res['tile_rows']} rows. Raw: search_rescore.json.", "",
             "## Time, launch to launch", "",
             f"Device events around {launches} back-to-back launch sequences; medians (us) over {rounds} rounds, every variant "
             "interleaved within each round; in brackets the spread (max - min) over the rounds. All rows live, no filter. "
             "`two-stage` = qscan + merge at k = R, then the rescore launch at k = 10; `device` / `host` is where the bf16 rows lie.", ""]
    names = list(res["speed"][0]["us_median"])
    lines += ["| variant | " + " | ".join(f"N = {c['N']}, Q = {c['Q']}" for c in res["speed"]) + " |",
              "|---|" + "---|" * len(res["speed"])]
    for n in names:
        lines.append(f"| {n} | " + " | ".join(f"{c['us_median'][n]} [{c['us_spread'][n]}]" for c in res["speed"]) + " |")
    lines += ["", "## Recall against fp64 truth over the unquantised vectors", "",
              "1e5 x 768 cosine rows, 1,000 queries drawn like the rows. `clusters`: 1,000 centres N(0, I), rows = centre + "
              "0.1 * N(0, I). recall@10 / recall@1.", "",
              "| corpus | " + " | ".join(n for n in res["quality"][0] if n not in ("corpus", "N", "queries", "k")) + " |",
              "|---|" + "---|" * 6]
    for c in res["quality"]:
        cols = [n for n in c if n not in ("corpus", "N", "queries", "k")]
        lines.append(f"| {c['corpus']} | " + " | ".join(f"{c[n]['recall_at_10']} / {c[n]['recall_at_1']}" for n in cols) + " |")
    lines += ["", "## Device bytes of an open index (1e5 x 768, two contexts)", "", "| index | device bytes |", "|---|---|"]
    lines += [f"| {n} | {b} |" for n, b in res["device_bytes"].items()]
    lines.append("")
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
