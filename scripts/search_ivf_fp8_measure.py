#!/usr/bin/env python3
"""The measurements of profiles/search_ivf_fp8/README.md on one MI355X; writes that file and search_ivf_fp8.json.

D = 768, k = 10, nlist = 1024, the method of scripts/search_ivf_measure.py: every comparison is interleaved round by
round on one box, launch to launch (device events around ``--launches`` back-to-back launch sequences), all rows
live, no filter; every step runs under its own time limit (SIGALRM).

1. Time, N in {1e5, 1e6} x Q in {1, 16} x nprobe in {1, 16, 64}, all sequences over the same vectors and lists:
   * version 5: scan + merge over the centroids at k = nprobe, list scan (kind 36), merge over P
   * version 6: the same with the quantised list scan (kind 37) over the e4m3 rows of the same stored rows
   * version 7 at R in {10, 40, 128}: kind 37 and its merge at k = R, then the rescore (kind 35) of those external ids
     against the bf16 rows held by id, in device memory and in mapped pinned host memory
   * for reference the plain two-stage sequence (kinds 34 + 32 at k = 128, then 35) and the plain bf16 scan (31 + 32)
2. Recall@10 and recall@1 against the fp64 truth over the unquantised vectors on the two corpora of
   scripts/search_fp8_measure.py (1e5 x 768 cosine rows, 1,000 queries) for versions 5, 6 and 7 at nprobe 1, 4, 16.
3. The device bytes ``describe()`` reports for the open indexes of one 1e5-row corpus (files written from the lists
   of step 2; version 7 in both placements).

The lists are built on the GPU (``search_ivf_measure.build_lists``); the e4m3 rows are the quantiser's arithmetic in
torch over the stored bf16 rows.

    python scripts/search_ivf_fp8_measure.py [--out profiles/search_ivf_fp8] [--rounds 7] [--launches 50] [--sizes 100000,1000000] [--iters 5]"""
import ctypes as C
import json
import os
import signal
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

from search_fp8_measure import DEV, D, K, _opt, _time  # noqa: E402
from search_ivf_measure import NLIST, T, Ivf, build_lists, corpus  # noqa: E402

PROBES = (1, 16, 64)
RECALL_PROBES = (1, 4, 16)
REFINES = (10, 40, 128)


class limit:
    """``with limit(seconds, what):`` -- the step ends the script if it runs longer."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _fire(self, *_):
        raise TimeoutError(f"{self.what}: over its limit of {self.seconds} s")

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


class HostRows:
    """bf16 rows in mapped pinned host memory, as the index places them (hipHostMallocMapped): ``ptr`` is what a
    kernel reads."""

    def __init__(self, rows):
        self.hip = OS.N.lib()  # the HIP runtime the library itself is linked against (dlsym follows its dependencies)
        host, dev = C.c_void_p(), C.c_void_p()
        nbytes = rows.numel() * 2
        self.hip.hipHostMalloc.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
        self.hip.hipHostGetDevicePointer.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        self.hip.hipHostFree.argtypes = [C.c_void_p]
        assert self.hip.hipHostMalloc(C.byref(host), nbytes, 2) == 0  # hipHostMallocMapped
        assert self.hip.hipHostGetDevicePointer(C.byref(dev), host, 0) == 0
        src = rows.cpu().contiguous().view(torch.int16).numpy()
        C.memmove(host, src.ctypes.data, nbytes)
        self.host, self.ptr = host, dev.value

    def free(self):
        self.hip.hipHostFree(self.host)


def quantise(stored, real):
    """Stored bf16 rows [cap, D] -> (codes uint8 [cap, D], scales fp32 [cap]); padding: code 0, scale 1."""
    codes = torch.zeros(stored.shape, dtype=torch.uint8, device=DEV)
    scales = torch.ones(stored.shape[0], dtype=torch.float32, device=DEV)
    for a in range(0, stored.shape[0], 65536):
        v = stored[a:a + 65536].float()
        amax = v.abs().amax(dim=1)
        s = torch.where(amax > 0, (amax / 448.0).clamp(min=torch.finfo(torch.float32).tiny), torch.ones_like(amax))
        codes[a:a + 65536] = (v / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        scales[a:a + 65536] = s
    keep = real.to(torch.uint8)
    return codes * keep[:, None], torch.where(real, scales, torch.ones_like(scales))


class Ivf8(Ivf):
    """``Ivf`` plus the e4m3 stored rows and the launches of versions 6 and 7 and of the plain two-stage index."""

    def __init__(self, bf, cb, assign, q):
        super().__init__(bf, cb, assign, q)
        stored = self.keep[2]
        real = torch.from_numpy(S.unpack_live(self.live_words, self.cap)).to(DEV)
        self.codes, self.scales = quantise(stored, real)
        self.pcodes, self.pscales = quantise(bf, torch.ones(bf.shape[0], dtype=torch.bool, device=DEV))  # the plain fp8 index
        self.mid_s, self.mid_i = torch.empty(self.Q, 128, device=DEV), torch.empty(self.Q, 128, dtype=torch.int32, device=DEV)
        self.host = None

    def ivf8(self, nprobe, R=0, host=False, k=K):
        """Version 6 (R = 0) or version 7 (stage one at k = R, then the rescore against the rows by id)."""
        bf, cb, _, q = self.keep
        P = self.budget(nprobe)
        cp = OS.SearchParams(cb.data_ptr(), q.data_ptr(), self.ccand.data_ptr(), self.psc.data_ptr(), self.pid.data_ptr(), NLIST,
                             D, self.Q, max(nprobe, 1), D, 0, self.ccand.numel() * 8)
        o_s, o_i = (self.mid_s, self.mid_i) if R else (self.sc, self.ids)
        lp = OS.QuantListScanParams(self.codes.data_ptr(), q.data_ptr(), self.cand.data_ptr(), o_s.data_ptr(), o_i.data_ptr(),
                                    self.cap, D, self.Q, R or k, D, 0, self.nbytes, self.lv.data_ptr(), 0, 0,
                                    self.live_words.size * 4, self.pid.data_ptr() if nprobe else 0,
                                    *(t.data_ptr() for t in self.tables), NLIST, nprobe, P, 0, self.scales.data_ptr())
        if host and self.host is None:
            self.host = HostRows(bf)
        rp = OS.RescoreParams(self.host.ptr if host else bf.data_ptr(), q.data_ptr(), self.mid_i.data_ptr(), self.sc.data_ptr(),
                              self.ids.data_ptr(), self.N, D, self.Q, max(R, 1), k, D)

        def run():
            rc = OS.launch(cp, self.st) if nprobe else (0, 0)
            rc2 = OS.launch_quant_list(lp, self.st)
            return (rc, rc2) if not R else (rc, rc2, OS.launch_rescore(rp, self.st))
        return run

    def plain_two_stage(self, R=128, k=K):
        bf, _, _, q = self.keep
        qp = OS.QuantScanParams(self.pcodes.data_ptr(), q.data_ptr(), self.cand.data_ptr(), self.mid_s.data_ptr(),
                                self.mid_i.data_ptr(), self.N, D, self.Q, R, D, 0, self.nbytes, self.lv_all.data_ptr(), 0, 0,
                                self.all_words.size * 4, self.pscales.data_ptr())
        rp = OS.RescoreParams(bf.data_ptr(), q.data_ptr(), self.mid_i.data_ptr(), self.sc.data_ptr(), self.ids.data_ptr(), self.N, D,
                              self.Q, R, k, D)
        return lambda: (OS.launch_quant(qp, self.st), OS.launch_rescore(rp, self.st))

    def result(self, fn, k=K):
        rc = fn()
        flat = [x for part in rc for x in (part if isinstance(part, tuple) else (part,))]
        assert all(x == 0 for x in flat), rc
        torch.cuda.synchronize()
        return self.ids.cpu().numpy().reshape(-1)[:self.Q * k].reshape(self.Q, k).copy()

    def close(self):
        if self.host is not None:
            self.host.free()
            self.host = None


def speed(N, rounds, launches, iters):
    with limit(240, f"lists for N = {N}"):
        bf = corpus("uniform", N, N)
        cb, assign = build_lists(bf, iters)
    g = torch.Generator(device=DEV).manual_seed(N + 1)
    out = []
    for Q in (1, 16):
        with limit(300, f"speed N = {N}, Q = {Q}"):
            q = torch.randn(Q, D, generator=g, device=DEV)
            q = q / q.norm(dim=1, keepdim=True)
            L = Ivf8(bf, cb, assign, q)
            runs = {"bf16 scan (31+32)": L.plain(False), "plain two-stage R=128 (34+32+35)": L.plain_two_stage()}
            for n in PROBES:
                runs[f"v5 nprobe={n}"] = L.ivf(n)
                runs[f"v6 nprobe={n}"] = L.ivf8(n)
                for R in REFINES:
                    runs[f"v7 nprobe={n} R={R} device"] = L.ivf8(n, R)
                    runs[f"v7 nprobe={n} R={R} host"] = L.ivf8(n, R, host=True)
            # every list and R = 128 reproduce the plain two-stage answer's ids or the run is not worth timing
            exact = L.result(L.plain(True))
            assert np.array_equal(L.result(L.ivf(0)), exact)
            two = L.result(L.plain_two_stage())
            assert np.array_equal(L.result(L.ivf8(0, 128)), two) and np.array_equal(L.result(L.ivf8(0, 128, host=True)), two)
            us = {n: [] for n in runs}
            for _ in range(rounds):
                for n, fn in runs.items():
                    us[n].append(_time(fn, launches))
            out.append({"N": N, "Q": Q, "rounds": rounds, "launches_per_round": launches, "tiles": L.ntile,
                        "P": {str(n): L.budget(n) for n in PROBES},
                        "us_median": {n: round(statistics.median(v), 1) for n, v in us.items()},
                        "us_spread": {n: round(max(v) - min(v), 1) for n, v in us.items()}})
            print(json.dumps(out[-1]), flush=True)
            L.close()
    return out


def quality(name, iters, N=100000, NQ=1000, seed=7):
    """The corpora of scripts/search_fp8_measure.py; recall of versions 5, 6 and 7 against the fp64 truth."""
    with limit(420, f"recall on {name}"):
        rng = np.random.default_rng(seed)
        if name == "isotropic":
            v, q = rng.standard_normal((N, D), dtype=np.float32), rng.standard_normal((NQ, D), dtype=np.float32)
        else:
            centres = rng.standard_normal((1000, D), dtype=np.float32)
            v = centres[rng.integers(0, 1000, N)] + np.float32(0.1) * rng.standard_normal((N, D), dtype=np.float32)
            q = centres[rng.integers(0, 1000, NQ)] + np.float32(0.1) * rng.standard_normal((NQ, D), dtype=np.float32)
        vn, qn = S.normalize_rows(v), S.normalize_rows(q)
        vd, qs = torch.from_numpy(vn).to(DEV), torch.from_numpy(qn).to(DEV)
        tid = torch.cat([(qs[a:a + 100].double() @ vd.double().T).topk(K, dim=1).indices for a in range(0, NQ, 100)]).cpu().numpy()
        bf = vd.to(torch.bfloat16)
        cb, assign = build_lists(bf, iters)
        kinds = {"v5": lambda L, n: L.ivf(n), "v6": lambda L, n: L.ivf8(n), "v7 R=40": lambda L, n: L.ivf8(n, 40),
                 "v7 R=128": lambda L, n: L.ivf8(n, 128)}
        hit10 = {(kind, n): 0 for kind in kinds for n in RECALL_PROBES + (0,)}
        hit1 = dict(hit10)
        L = None
        for a in range(0, NQ, 16):
            qb = qs[a:a + 16].contiguous()
            if L is None or qb.shape[0] != L.Q:
                L = Ivf8(bf, cb, assign, qb)
            else:
                L.keep = L.keep[:3] + (qb,)
            for kind, make in kinds.items():
                for n in RECALL_PROBES + (0,):
                    got = L.result(make(L, n))
                    want = tid[a:a + 16]
                    hit10[(kind, n)] += sum(len(set(g_) & set(e)) for g_, e in zip(got.tolist(), want.tolist()))
                    hit1[(kind, n)] += int((got[:, 0] == want[:, 0]).sum())
        out = {"corpus": name, "N": N, "queries": NQ,
               "recall_at_10": {kind: {str(n or "all"): round(hit10[(kind, n)] / (NQ * K), 4) for n in RECALL_PROBES + (0,)} for kind in kinds},
               "recall_at_1": {kind: {str(n or "all"): round(hit1[(kind, n)] / NQ, 4) for n in RECALL_PROBES + (0,)} for kind in kinds}}
        print(json.dumps(out), flush=True)
    return out, (bf, cb, assign)


def device_bytes(bf, cb, assign):
    """Files of the 1e5-row corpus written from the GPU-built lists -> what ``describe()`` reports per open index."""
    with limit(420, "device bytes"):
        bits = bf.cpu().view(torch.int16).numpy().view(np.uint16)
        N = bits.shape[0]
        lay = S.ivf_layout(assign.astype(np.int64), NLIST)
        real = lay["rowid"] >= 0
        srows = np.zeros((real.size, D), np.uint16)
        srows[real] = bits[lay["rowid"][real]]
        lay.update(centroids=cb.cpu().view(torch.int16).numpy().view(np.uint16), nlist=NLIST, nprobe=16, seed=0, iters=0)
        hdr = {"dim": D, "count": N, "dtype": "bf16", "metric": "cosine", "model": "", "embed": None}
        out = {}
        with tempfile.TemporaryDirectory() as d:
            p = {k: os.path.join(d, k + ".hzidx") for k in ("v1", "v4", "v5", "v6", "v7")}
            S._write_file(p["v1"], dict(hdr), bits)
            S._write_file(p["v5"], dict(hdr), srows, np.zeros(real.size, np.uint32), real, ivf=lay)
            S.convert_index(p["v1"], p["v4"], "fp8", rescore=True)
            S.convert_index(p["v5"], p["v6"], "fp8")
            S.convert_index(p["v5"], p["v7"], "fp8", rescore=True)
            for name, key, kw in (("plain bf16 (version 1)", "v1", {}), ("plain two-stage (version 4), device rows", "v4", {}),
                                  ("plain two-stage (version 4), host rows", "v4", {"rescore_rows": "host"}),
                                  ("IVF bf16 (version 5)", "v5", {}), ("IVF fp8 (version 6)", "v6", {}),
                                  ("IVF two-stage (version 7), device rows", "v7", {}),
                                  ("IVF two-stage (version 7), host rows", "v7", {"rescore_rows": "host"})):
                with S.Index(p[key], contexts=1, **kw) as ix:
                    out[name] = {"device_bytes": ix.describe()["device_bytes"], "file_bytes": os.path.getsize(p[key])}
        tiles = real.size // T
        out["ivf tables and centroids (not in device_bytes)"] = {"device_bytes": NLIST * D * 2 + (NLIST + 1 + tiles + real.size) * 4,
                                                                 "file_bytes": 0}
    return out


def main():
    out_dir = _opt("--out", "profiles/search_ivf_fp8", str)
    rounds, launches, iters = _opt("--rounds", 7), _opt("--launches", 50), _opt("--iters", 5)
    sizes = [int(x) for x in _opt("--sizes", "100000,1000000", str).split(",")]
    os.makedirs(out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "D": D, "k": K, "nlist": NLIST, "kmeans_iters": iters,
           "speed": [r for N in sizes for r in speed(N, rounds, launches, iters)], "recall": []}
    keep = None
    for name in ("isotropic", "clusters"):
        r, keep = quality(name, iters)
        res["recall"].append(r)
    res["device_bytes"] = device_bytes(*keep)
    json.dump(res, open(os.path.join(out_dir, "search_ivf_fp8.json"), "w"), indent=1)
    lines = ["# fp8 IVF indexes and two-stage IVF search against the existing programs (scripts/search_ivf_fp8_measure.py)", "",
             f"{res['device']}, D = {D}, k = {K}, nlist = {NLIST}, k-means rounds = {iters}; medians of {rounds} interleaved rounds of "
             f"{launches} back-to-back launch sequences, device events, microseconds per sequence (spread = max - min of the rounds).", ""]
    for r in res["speed"]:
        lines += [f"## N = {r['N']}, Q = {r['Q']} ({r['tiles']} tiles; P at nprobe 1 / 16 / 64 = "
                  + " / ".join(str(r["P"][str(n)]) for n in PROBES) + ")", "",
                  f"bf16 scan (31+32): {r['us_median']['bf16 scan (31+32)']} ({r['us_spread']['bf16 scan (31+32)']}); plain two-stage "
                  f"R=128 (34+32+35): {r['us_median']['plain two-stage R=128 (34+32+35)']} "
                  f"({r['us_spread']['plain two-stage R=128 (34+32+35)']})", "",
                  "| nprobe | v5 | v6 | " + " | ".join(f"v7 R={R} {pl}" for R in REFINES for pl in ("device", "host")) + " |",
                  "|---|---|---|" + "---|" * (2 * len(REFINES))]
        for n in PROBES:
            cols = [f"v5 nprobe={n}", f"v6 nprobe={n}"] + [f"v7 nprobe={n} R={R} {pl}" for R in REFINES for pl in ("device", "host")]
            lines.append(f"| {n} | " + " | ".join(f"{r['us_median'][c]} ({r['us_spread'][c]})" for c in cols) + " |")
        lines.append("")
    for key, title in (("recall_at_10", "Recall@10"), ("recall_at_1", "Recall@1")):
        lines += [f"{title} against the fp64 truth over the unquantised vectors, 1e5 x 768 cosine rows, 1,000 queries:", "",
                  "| corpus | index | " + " | ".join(f"nprobe {n}" for n in RECALL_PROBES) + " | all lists |", "|---|---|" + "---|" * (len(RECALL_PROBES) + 1)]
        for r in res["recall"]:
            for kind, row in r[key].items():
                lines.append(f"| {r['corpus']} | {kind} | " + " | ".join(str(row[str(n)]) for n in RECALL_PROBES) + f" | {row['all']} |")
        lines.append("")
    lines += ["Device bytes of the open indexes of the clustered 1e5-row corpus (one context), and their files:", "",
              "| index | device bytes | file bytes |", "|---|---|---|"]
    lines += [f"| {n} | {b['device_bytes']} | {b['file_bytes']} |" for n, b in res["device_bytes"].items()]
    lines += ["", "No threshold is set on any of these numbers: they are findings.", ""]
    open(os.path.join(out_dir, "README.md"), "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
