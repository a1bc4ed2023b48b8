#!/usr/bin/env python3
"""The measurements of profiles/search_ivf/README.md on one MI355X; writes that file and search_ivf.json.

D = 768, k = 10, nlist = 1024. Every comparison is interleaved round by round on one box, launch to launch (device
events around ``--launches`` back-to-back launch sequences), all rows live, no filter.

1. Time, N in {1e5, 1e6} x Q in {1, 16}: the IVF sequence -- scan + merge over the centroids at k = nprobe, list scan
   with P = the tiles of the nprobe largest lists, merge over P -- at nprobe 1, 4, 16, 64, and the list scan over
   every list ("all": no coarse stage), against scan + merge (kinds 31 + 32) and filtered scan + merge (kinds
   33 + 32) over the same vectors in their original order.
2. Recall@10 against the exact answer (the same kernels over every list) per nprobe, 1e5 x 768 cosine rows, 1,000
   queries: a clustered corpus (1,000 clusters, sigma 0.1; queries near corpus rows) and a uniform one (isotropic
   rows and queries: the worst case, no structure to find).

The lists are built on the GPU by this script (the arithmetic of ``hipzap.search.ivf_kmeans`` in torch: at most 256
sample rows per centroid, ``--iters`` rounds, assignment by the largest inner product with the bf16-rounded
centroids) and laid out by ``hipzap.search.ivf_layout``; numpy's k-means over 1e6 x 768 x 1024 is minutes of CPU.

    python scripts/search_ivf_measure.py [--out profiles/search_ivf] [--rounds 7] [--launches 50] [--sizes 100000,1000000] [--iters 5]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

from search_fp8_measure import DEV, D, K, _dev_u32, _opt, _time  # noqa: E402

NLIST = 1024
PROBES = (1, 4, 16, 64)
T = 256


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def build_lists(bf, iters, seed=0):
    """bf16 unit rows [N, D] on the device -> (centroids bf16 [NLIST, D], assign int64 [N] on the host)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = bf.shape[0]
    m = min(N, S.IVF_SAMPLE * NLIST)
    sample = bf[torch.randperm(N, generator=g, device=DEV)[:m]].float()
    cent = sample[torch.randperm(m, generator=g, device=DEV)[:NLIST]].clone()
    for _ in range(iters):
        a = (sample @ cent.to(torch.bfloat16).float().T).argmax(dim=1)
        sums = torch.zeros_like(cent).index_add_(0, a, sample)
        cnt = torch.bincount(a, minlength=NLIST)
        mean = sums / cnt.clamp(min=1)[:, None]
        mean = mean / mean.norm(dim=1, keepdim=True).clamp(min=1e-12)
        cent = torch.where((cnt > 0)[:, None], mean, cent)
    cb = cent.to(torch.bfloat16)
    assign = torch.empty(N, dtype=torch.int64, device=DEV)
    for s in range(0, N, 65536):
        assign[s:s + 65536] = (bf[s:s + 65536].float() @ cb.float().T).argmax(dim=1)
    return cb, assign.cpu().numpy()


class Ivf:
    """The launches over one corpus (original order and IVF order) for a given query block."""

    def __init__(self, bf, cb, assign, q):
        N, Q = bf.shape[0], q.shape[0]
        lay = S.ivf_layout(assign, NLIST)
        rowid = lay["rowid"]
        cap = rowid.size
        self.N, self.Q, self.cap, self.ntile = N, Q, cap, cap // T
        stored = torch.zeros(cap, D, dtype=torch.bfloat16, device=DEV)
        real = torch.from_numpy(rowid >= 0).to(DEV)
        stored[real] = bf[torch.from_numpy(rowid[rowid >= 0].astype(np.int64)).to(DEV)]
        self.tiles_desc = np.sort(np.diff(lay["list_off"]))[::-1]
        self.sizes = np.bincount(assign, minlength=NLIST)
        self.live_words, self.all_words = S.pack_live(rowid >= 0), S.pack_live(np.ones(N, bool))
        self.lv, self.lv_all = _dev_u32(self.live_words), _dev_u32(self.all_words)
        self.tables = [_i32(lay["list_off"]), _i32(lay["list_tiles"]), _i32(rowid)]
        self.nbytes = max(OS.scratch_bytes(cap, Q, 128), OS.scratch_bytes(N, Q, 128))
        self.cand = torch.zeros(self.nbytes // 8, dtype=torch.int64, device=DEV)
        self.ccand = torch.zeros(OS.scratch_bytes(NLIST, Q, 128) // 8, dtype=torch.int64, device=DEV)
        self.sc, self.ids = torch.empty(Q, 128, device=DEV), torch.empty(Q, 128, dtype=torch.int32, device=DEV)
        self.psc, self.pid = torch.empty(Q, 128, device=DEV), torch.empty(Q, 128, dtype=torch.int32, device=DEV)
        self.keep = (bf, cb, stored, q)
        self.st = torch.cuda.current_stream().cuda_stream

    def plain(self, filtered, k=K):
        bf, _, _, q = self.keep
        head = (bf.data_ptr(), q.data_ptr(), self.cand.data_ptr(), self.sc.data_ptr(), self.ids.data_ptr(), self.N, D, self.Q, k,
                D, 0, self.nbytes)
        if filtered:
            p = OS.FilterScanParams(*head, self.lv_all.data_ptr(), 0, 0, self.all_words.size * 4)
            return lambda: OS.launch_filtered(p, self.st)
        p = OS.SearchParams(*head)
        return lambda: OS.launch(p, self.st)

    def budget(self, nprobe):
        return int(self.tiles_desc[:nprobe].sum()) if nprobe else self.ntile

    def ivf(self, nprobe, k=K):
        """nprobe = 0: every list."""
        _, cb, stored, q = self.keep
        P = self.budget(nprobe)
        cp = OS.SearchParams(cb.data_ptr(), q.data_ptr(), self.ccand.data_ptr(), self.psc.data_ptr(), self.pid.data_ptr(), NLIST,
                             D, self.Q, max(nprobe, 1), D, 0, self.ccand.numel() * 8)
        lp = OS.ListScanParams(stored.data_ptr(), q.data_ptr(), self.cand.data_ptr(), self.sc.data_ptr(), self.ids.data_ptr(),
                               self.cap, D, self.Q, k, D, 0, self.nbytes, self.lv.data_ptr(), 0, 0, self.live_words.size * 4,
                               self.pid.data_ptr() if nprobe else 0, *(t.data_ptr() for t in self.tables), NLIST, nprobe, P, 0)

        def run():
            rc = OS.launch(cp, self.st) if nprobe else (0, 0)
            return rc, OS.launch_list(lp, self.st)
        return run

    def result(self, fn, k=K):
        rc = fn()
        assert rc in ((0, 0), ((0, 0), (0, 0))), rc
        torch.cuda.synchronize()
        return self.ids.cpu().numpy().reshape(-1)[:self.Q * k].reshape(self.Q, k).copy()


def corpus(name, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if name == "uniform":
        v = torch.randn(N, D, generator=g, device=DEV)
    else:
        cent = torch.randn(1000, D, generator=g, device=DEV)
        cent = cent / cent.norm(dim=1, keepdim=True)
        v = cent[torch.randint(0, 1000, (N,), generator=g, device=DEV)] + 0.1 / D ** 0.5 * torch.randn(N, D, generator=g, device=DEV)
    return (v / v.norm(dim=1, keepdim=True)).to(torch.bfloat16)


def speed(N, rounds, launches, iters):
    bf = corpus("uniform", N, N)
    cb, assign = build_lists(bf, iters)
    g = torch.Generator(device=DEV).manual_seed(N + 1)
    out = []
    for Q in (1, 16):
        q = torch.randn(Q, D, generator=g, device=DEV)
        q = q / q.norm(dim=1, keepdim=True)
        L = Ivf(bf, cb, assign, q)
        runs = {"scan+merge (31+32)": L.plain(False), "fscan+merge (33+32)": L.plain(True)}
        for n in PROBES:
            runs[f"ivf nprobe={n}"] = L.ivf(n)
        runs["ivf all lists"] = L.ivf(0)
        exact = L.result(L.plain(True))
        assert np.array_equal(L.result(L.ivf(0)), exact), "every list must give the exact answer"
        us = {n: [] for n in runs}
        for _ in range(rounds):
            for n, fn in runs.items():
                us[n].append(_time(fn, launches))
        out.append({"N": N, "Q": Q, "rounds": rounds, "launches_per_round": launches, "tiles": L.ntile,
                    "padding_rows": L.cap - N, "largest_list": int(L.sizes.max()), "empty_lists": int((L.sizes == 0).sum()),
                    "P": {str(n): L.budget(n) for n in PROBES + (0,)},
                    "us_median": {n: round(statistics.median(v), 1) for n, v in us.items()},
                    "us_spread": {n: round(max(v) - min(v), 1) for n, v in us.items()}})
        print(json.dumps(out[-1]), flush=True)
    return out


def recall(name, iters, N=100000, NQ=1000, seed=7):
    bf = corpus(name, N, seed)
    cb, assign = build_lists(bf, iters)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    if name == "uniform":
        qs = torch.randn(NQ, D, generator=g, device=DEV)
    else:
        qs = bf[torch.randint(0, N, (NQ,), generator=g, device=DEV)].float() + 0.05 * torch.randn(NQ, D, generator=g, device=DEV) / D ** 0.5
    qs = qs / qs.norm(dim=1, keepdim=True)
    hits, total = {n: 0 for n in PROBES}, 0
    L = None
    for a in range(0, NQ, 16):
        q = qs[a:a + 16].contiguous()
        if L is None or q.shape[0] != L.Q:
            L = Ivf(bf, cb, assign, q)
        else:
            L.keep = L.keep[:3] + (q,)
        exact = L.result(L.ivf(0))
        total += exact.size
        for n in PROBES:
            got = L.result(L.ivf(n))
            hits[n] += sum(len(set(g_) & set(e)) for g_, e in zip(got.tolist(), exact.tolist()))
    sizes = np.bincount(assign, minlength=NLIST)
    out = {"corpus": name, "N": N, "queries": NQ, "largest_list": int(sizes.max()), "empty_lists": int((sizes == 0).sum()),
           "recall_at_10": {str(n): round(hits[n] / total, 4) for n in PROBES}}
    print(json.dumps(out), flush=True)
    return out


def main():
    out_dir = _opt("--out", "profiles/search_ivf", str)
    rounds, launches, iters = _opt("--rounds", 7), _opt("--launches", 50), _opt("--iters", 5)
    sizes = [int(x) for x in _opt("--sizes", "100000,1000000", str).split(",")]
    os.makedirs(out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "D": D, "k": K, "nlist": NLIST, "kmeans_iters": iters,
           "speed": [r for N in sizes for r in speed(N, rounds, launches, iters)],
           "recall": [recall(name, iters) for name in ("clustered", "uniform")]}
    json.dump(res, open(os.path.join(out_dir, "search_ivf.json"), "w"), indent=1)
    names = list(res["speed"][0]["us_median"])
    lines = ["# IVF indexes: list scan + coarse stage against the full scans (scripts/search_ivf_measure.py)", "",
             f"{res['device']}, D = {D}, k = {K}, nlist = {NLIST}, k-means rounds = {iters}; medians of {rounds} interleaved rounds of "
             f"{launches} back-to-back launch sequences, device events, microseconds per sequence (spread = max - min of the rounds).",
             "", "| N | Q | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
    for r in res["speed"]:
        lines.append(f"| {r['N']} | {r['Q']} | " + " | ".join(f"{r['us_median'][n]} ({r['us_spread'][n]})" for n in names) + " |")
    lines += ["", "Tile budgets P (workgroup columns of the list scan; the grid is P x Q) and the lists:", "",
              "| N | tiles | padding rows | largest list | empty lists | P at nprobe 1 / 4 / 16 / 64 |", "|---|---|---|---|---|---|"]
    for r in res["speed"][::2]:
        lines.append(f"| {r['N']} | {r['tiles']} | {r['padding_rows']} | {r['largest_list']} | {r['empty_lists']} | "
                     + " / ".join(str(r["P"][str(n)]) for n in PROBES) + " |")
    lines += ["", "Recall@10 against the exact answer (every list), 1e5 x 768 cosine rows, 1,000 queries:", "",
              "| corpus | largest list | empty lists | " + " | ".join(f"nprobe {n}" for n in PROBES) + " |", "|---|---|---|" + "---|" * len(PROBES)]
    for r in res["recall"]:
        lines.append(f"| {r['corpus']} | {r['largest_list']} | {r['empty_lists']} | "
                     + " | ".join(str(r["recall_at_10"][str(n)]) for n in PROBES) + " |")
    lines += ["", "\"ivf all lists\" against \"fscan+merge\" is the price of the indirection, of Q workgroups per tile and of the "
              "padding rows' tiles: a finding, not a gate.", ""]
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
