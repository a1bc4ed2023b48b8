#!/usr/bin/env python3
"""The measurements of profiles/search_fp8/README.md on one MI355X; writes that file and search_fp8.json.

D = 768, k = 10. Every comparison is interleaved round by round on one box.

1. Speed, launch to launch (device events around ``--launches`` back-to-back pairs): fscan + merge (kinds 33 + 32)
   over a bf16 corpus against qscan + merge (kinds 34 + 32) over the fp8 corpus of the same vectors, all rows live,
   no filter, N in {1e5, 1e6} and Q in {1, 16}; at the largest N also with a tag filter that passes 1 % of the rows.
   Both are kernels of the library that is loaded and run in the same process. Achieved bytes/s count the row block (and the scales) once.
2. Quality: recall@10 and the mean absolute score error of the fp8 index and of the bf16 index against the fp64
   truth over the unquantised, normalised fp32 vectors: 1e5 x 768 cosine rows, 1,000 queries drawn like the rows;
   an isotropic Gaussian corpus, and 1,000 Gaussian clusters (centres N(0, I), rows = centre + 0.1 * N(0, I)).

    python scripts/search_fp8_measure.py [--out profiles/search_fp8] [--rounds 7] [--launches 50] [--sizes 100000,1000000]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

DEV = "cuda:0"
D, K = 768, 10


def _opt(flag, default, cast=int):
    return cast(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def _time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per call


def _dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def device_corpora(N, seed):
    """Unit rows on the device as bf16 and as (e4m3fn codes, scales): the quantiser's arithmetic in torch."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    bf = torch.empty(N, D, dtype=torch.bfloat16, device=DEV)
    codes = torch.empty(N, D, dtype=torch.uint8, device=DEV)
    scales = torch.empty(N, dtype=torch.float32, device=DEV)
    for a in range(0, N, 65536):
        v = torch.randn(min(65536, N - a), D, generator=g, device=DEV)
        v = v / v.norm(dim=1, keepdim=True)
        s = v.abs().amax(dim=1) / 448.0
        bf[a:a + v.shape[0]] = v.to(torch.bfloat16)
        codes[a:a + v.shape[0]] = (v / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        scales[a:a + v.shape[0]] = s
    return bf, codes, scales


class Launcher:
    """The two launches over one pair of corpora with shared outputs, for a given Q."""

    def __init__(self, bf, codes, scales, q, tags=None, filt=None, k=K):
        N, Q = bf.shape[0], q.shape[0]
        self.nbytes = OS.scratch_bytes(N, Q, k)
        self.cand = torch.zeros(self.nbytes // 8, dtype=torch.int64, device=DEV)
        self.sc = torch.empty(Q, k, device=DEV)
        self.ids = torch.empty(Q, k, dtype=torch.int32, device=DEV)
        self.words = S.pack_live(np.ones(N, bool))
        self.lv = _dev_u32(self.words)
        self.keep = (bf, codes, scales, q, tags, filt)
        self.st = torch.cuda.current_stream().cuda_stream
        tail = (self.lv.data_ptr(), tags.data_ptr() if tags is not None else 0, filt.data_ptr() if filt is not None else 0,
                self.words.size * 4)
        out = (self.cand.data_ptr(), self.sc.data_ptr(), self.ids.data_ptr(), N, D, Q, k, D, 0, self.nbytes)
        self.fp = OS.FilterScanParams(bf.data_ptr(), q.data_ptr(), *out, *tail)
        self.qp = OS.QuantScanParams(codes.data_ptr(), q.data_ptr(), *out, *tail, scales.data_ptr())

    def bf16(self):
        return OS.launch_filtered(self.fp, self.st)

    def fp8(self):
        return OS.launch_quant(self.qp, self.st)

    def result(self, fn):
        assert fn() == (0, 0)
        torch.cuda.synchronize()
        return self.sc.cpu().numpy().copy(), self.ids.cpu().numpy().copy()


def speed(N, rounds, launches, with_tag):
    bf, codes, scales = device_corpora(N, N)
    g = torch.Generator(device=DEV).manual_seed(N + 1)
    out = []
    cases = [(1, False), (16, False)] + ([(1, True)] if with_tag else [])
    for Q, tagged in cases:
        q = torch.randn(Q, D, generator=g, device=DEV)
        q = q / q.norm(dim=1, keepdim=True)
        tags = _dev_u32(np.arange(N) % 100) if tagged else None
        filt = _dev_u32(np.tile(np.array([[0xFFFFFFFF, 7]]), (Q, 1))) if tagged else None
        L = Launcher(bf, codes, scales, q, tags, filt)
        rb, rq = L.result(L.bf16), L.result(L.fp8)
        if tagged:
            assert (rb[1] % 100 == 7).all() and (rq[1] % 100 == 7).all()
        overlap = float(np.mean([len(set(a) & set(b)) / K for a, b in zip(rb[1], rq[1])]))
        us = {"bf16": [], "fp8": []}
        for _ in range(rounds):
            us["bf16"].append(_time(L.bf16, launches))
            us["fp8"].append(_time(L.fp8, launches))
        med = {n: statistics.median(v) for n, v in us.items()}
        frac = 0.01 if tagged else 1.0
        out.append({"N": N, "Q": Q, "tag_filter_1pct": tagged, "rounds": rounds, "launches_per_round": launches,
                    "us": {n: [round(x, 1) for x in v] for n, v in us.items()},
                    "us_median": {n: round(v, 1) for n, v in med.items()},
                    "us_spread": {n: round(max(v) - min(v), 1) for n, v in us.items()},
                    "speedup": round(med["bf16"] / med["fp8"], 3),
                    "TBps": {"bf16": round(frac * N * D * 2 / med["bf16"] / 1e6, 3),
                             "fp8": round(frac * N * (D + 4) / med["fp8"] / 1e6, 3)},
                    "top10_overlap_bf16_fp8": round(overlap, 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


def quality(name, N=100000, NQ=1000, seed=7):
    rng = np.random.default_rng(seed)
    if name == "isotropic":
        v, q = rng.standard_normal((N, D), dtype=np.float32), rng.standard_normal((NQ, D), dtype=np.float32)
    else:
        centres = rng.standard_normal((1000, D), dtype=np.float32)
        v = centres[rng.integers(0, 1000, N)] + np.float32(0.1) * rng.standard_normal((N, D), dtype=np.float32)
        q = centres[rng.integers(0, 1000, NQ)] + np.float32(0.1) * rng.standard_normal((NQ, D), dtype=np.float32)
    vn, qn = S.normalize_rows(v), S.normalize_rows(q)
    truth = torch.from_numpy(qn).to(DEV).double() @ torch.from_numpy(vn).to(DEV).double().T  # fp64 [NQ, N]
    tid = truth.topk(K, dim=1).indices.cpu().numpy()
    bits = S.prepare_rows(v, "cosine")
    codes, scales = S.prepare_rows_fp8(v, "cosine")
    bf = torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.bfloat16)
    cd, sd = torch.from_numpy(codes).to(DEV), torch.from_numpy(scales).to(DEV)
    got = {"bf16": [], "fp8": []}
    for a in range(0, NQ, 16):
        L = Launcher(bf, cd, sd, torch.from_numpy(qn[a:a + 16]).to(DEV))
        got["bf16"].append(L.result(L.bf16))
        got["fp8"].append(L.result(L.fp8))
    out = {"corpus": name, "N": N, "queries": NQ, "k": K}
    for n, parts in got.items():
        sc, ids = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        exact = truth.gather(1, torch.from_numpy(ids.astype(np.int64)).to(DEV)).cpu().numpy()
        out[n] = {"recall_at_10": round(float(np.mean([len(set(a) & set(b)) / K for a, b in zip(ids, tid)])), 4),
                  "recall_at_1": round(float(np.mean(ids[:, 0] == tid[:, 0])), 4),
                  "mean_abs_score_error": float(np.abs(sc.astype(np.float64) - exact).mean())}
    print(json.dumps(out), flush=True)
    return out


def main():
    out_dir = _opt("--out", "profiles/search_fp8", str)
    rounds, launches = _opt("--rounds", 7), _opt("--launches", 50)
    sizes = [int(x) for x in _opt("--sizes", "100000,1000000", str).split(",")]
    os.makedirs(out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tile_rows": OS.tile_rows(), "D": D, "k": K,
           "speed": [], "quality": []}
    for N in sizes:
        res["speed"] += speed(N, rounds, launches, with_tag=N == max(sizes))
    for name in ("isotropic", "clusters"):
        res["quality"].append(quality(name))
    with open(os.path.join(out_dir, "search_fp8.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["# fp8 indexes: qscan over e4m3 rows against fscan over bf16 rows (scripts/search_fp8_measure.py)", "",
             f"Device: {res['device']}, torch {res['torch']}. D = {D}, k = {K}, tile = {res['tile_rows']} rows. Raw: search_fp8.json.", "",
             "## Speed, launch to launch", "",
             f"Device events around {launches} back-to-back (scan, merge) pairs; medians over {rounds} rounds, the two corpora "
             "interleaved within each round; in brackets the spread (max - min) over the rounds. All rows live. TB/s counts "
             "the rows a launch has to read (N x D x 2 bytes; N x (D + 4) for fp8; 1 % of that under the tag filter). The "
             "unfiltered bf16 scan reached 4.69 TB/s at N = 1e6, Q = 1 (DESIGN.md 4l).", "",
             "| N | Q | filter | bf16 fscan + merge (us) | fp8 qscan + merge (us) | bf16 / fp8 | bf16 TB/s | fp8 TB/s |",
             "|---|---|---|---|---|---|---|---|"]
    for c in res["speed"]:
        m, sp = c["us_median"], c["us_spread"]
        lines.append(f"| {c['N']} | {c['Q']} | {'tag, 1 % pass' if c['tag_filter_1pct'] else 'none'} | {m['bf16']} [{sp['bf16']}] | "
                     f"{m['fp8']} [{sp['fp8']}] | {c['speedup']}x | {c['TBps']['bf16']} | {c['TBps']['fp8']} |")
    lines += ["", "## Quality against fp64 truth over the unquantised vectors", "",
              "1e5 x 768 cosine rows, 1,000 queries drawn like the rows. `clusters`: 1,000 centres N(0, I), rows = centre + "
              "0.1 * N(0, I).", "",
              "| corpus | bf16 recall@10 | fp8 recall@10 | bf16 recall@1 | fp8 recall@1 | bf16 mean abs score error | fp8 mean abs score error |",
              "|---|---|---|---|---|---|---|"]
    for c in res["quality"]:
        lines.append(f"| {c['corpus']} | {c['bf16']['recall_at_10']} | {c['fp8']['recall_at_10']} | {c['bf16']['recall_at_1']} | "
                     f"{c['fp8']['recall_at_1']} | {c['bf16']['mean_abs_score_error']:.2e} | {c['fp8']['mean_abs_score_error']:.2e} |")
    lines.append("")
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
