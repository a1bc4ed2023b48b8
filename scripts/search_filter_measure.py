#!/usr/bin/env python3
"""The measurements of profiles/search_filter/README.md on one MI355X; writes that file with its raw JSON.

D = 768, k = 10, Q = 1, N in {1e5, 1e6}. Every comparison is interleaved round by round on one box.

1. Kernels, launch to launch (device events around ``--launches`` back-to-back pairs): the unfiltered scan +
   merge (kinds 31 + 32) against fscan + merge (kinds 33 + 32), both of the library that is loaded, with
   all rows live and no filter; half the rows dead at random; half the rows dead as whole tiles (a random half
   of the tiles, and every other tile: consecutive workgroups go to the 8 XCDs in turn, so that pattern leaves
   the live tiles on half of them); all rows live and a tag filter that passes 1 % of them.
2. The index: ``search`` wall time of a never-mutated index (the unfiltered program) against the same file
   after one ``delete`` (the filtered program); ``add`` of 1 row (inside the last tile: device data only) and
   of 256 rows (crosses a tile boundary: the programs are destroyed); the first search after such an add
   (build, eager run, capture) and the one after it (replay).

    python scripts/search_filter_measure.py [--out profiles/search_filter] [--rounds 7] [--launches 50] [--sizes 100000,1000000]"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipzap import search as S  # noqa: E402
from hipzap.ops import search as OS  # noqa: E402

DEV = "cuda:0"
D, K, Q = 768, 10, 1
VARIANTS = ("scan", "all_live", "half_dead_random", "half_dead_tiles", "half_dead_tiles_alternate", "tag_1pct")


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


def kernels(N, rounds, launches):
    T = OS.tile_rows()
    g = torch.Generator(device=DEV).manual_seed(N)
    corpus = torch.randn(N, D, generator=g, device=DEV).to(torch.bfloat16)
    q = torch.randn(Q, D, generator=g, device=DEV)
    nbytes = OS.scratch_bytes(N, Q, K)
    cand = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    sc = torch.empty(Q, K, device=DEV)
    ids = torch.empty(Q, K, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(N)
    lives = {"all_live": np.ones(N, bool), "half_dead_random": rng.random(N) < 0.5,
             "half_dead_tiles": (rng.random(-(-N // T)) < 0.5)[np.arange(N) // T],
             "half_dead_tiles_alternate": (np.arange(N) // T) % 2 == 0, "tag_1pct": np.ones(N, bool)}
    tags = _dev_u32(np.arange(N) % 100)
    filt = _dev_u32(np.array([[0xFFFFFFFF, 7]]))
    keep = []  # device buffers the parameter blocks point to
    base = (corpus.data_ptr(), q.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(), N, D, Q, K, D, 0, nbytes)
    sp = OS.SearchParams(*base)
    fns = {"scan": lambda: OS.launch(sp, st)}
    for name, live in lives.items():
        words = S.pack_live(live)
        lv = _dev_u32(words)
        keep.append(lv)
        tagged = name == "tag_1pct"
        fp = OS.FilterScanParams(*base, lv.data_ptr(), tags.data_ptr() if tagged else 0, filt.data_ptr() if tagged else 0,
                                 words.size * 4)
        fns[name] = (lambda fp=fp: OS.launch_filtered(fp, st))
    want = {}
    for name, fn in fns.items():  # what is timed is also right: ids against the unfiltered run's, restricted
        assert fn() == (0, 0), name
        torch.cuda.synchronize()
        want[name] = ids.cpu().numpy().copy()
    assert np.array_equal(want["scan"], want["all_live"])
    for name in ("half_dead_random", "half_dead_tiles", "half_dead_tiles_alternate"):
        assert lives[name][want[name]].all(), name
    assert (want["tag_1pct"] % 100 == 7).all()
    us = {name: [] for name in VARIANTS}
    for _ in range(rounds):
        for name in VARIANTS:
            us[name].append(_time(fns[name], launches))
    med = {name: statistics.median(v) for name, v in us.items()}
    return {"N": N, "Q": Q, "D": D, "k": K, "rounds": rounds, "launches_per_round": launches,
            "us": {n: [round(x, 1) for x in v] for n, v in us.items()},
            "us_median": {n: round(v, 1) for n, v in med.items()},
            "us_spread": {n: round(max(v) - min(v), 1) for n, v in us.items()},
            "over_scan": {n: round(med[n] / med["scan"], 3) for n in VARIANTS},
            "live_fraction": {n: round(float(v.mean()), 4) for n, v in lives.items()}}


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def index(N, rounds, launches):
    rng = np.random.default_rng(N + 1)
    root = tempfile.mkdtemp(prefix="hz-filter-")
    path = os.path.join(root, "c.hzidx")
    S.write_index(path, rng.standard_normal((N, D), dtype=np.float32), "ip")
    q = rng.standard_normal((Q, D), dtype=np.float32)
    one, many = rng.standard_normal((1, D), dtype=np.float32), rng.standard_normal((256, D), dtype=np.float32)
    out = {"N": N, "search_unfiltered_us": [], "search_filtered_us": []}
    with S.Index(path, contexts=1) as plain, S.Index(path, contexts=1, reserve=N + 8192) as live:
        assert live.delete([0]) == 1 and live.describe()["filtered"] and not plain.describe()["filtered"]
        for ix in (plain, live):
            for _ in range(5):
                ix.search(q, K)
        for _ in range(rounds):
            for ix, key in ((plain, "search_unfiltered_us"), (live, "search_filtered_us")):
                out[key].append(round(statistics.median(_wall(lambda: ix.search(q, K)) for _ in range(launches)), 1))
        progs = live.describe()["programs"]
        out["add_1_us"] = [round(_wall(lambda: live.add(one)), 1) for _ in range(20)]  # N % 256 leaves room for 20 rows
        assert live.describe()["programs"] == progs
        out["add_256_us"], out["first_search_after_recapture_us"], out["next_search_us"] = [], [], []
        for _ in range(10):
            out["add_256_us"].append(round(_wall(lambda: live.add(many)), 1))
            assert live.describe()["programs"] == 0  # a tile boundary was crossed
            out["first_search_after_recapture_us"].append(round(_wall(lambda: live.search(q, K)), 1))
            out["next_search_us"].append(round(_wall(lambda: live.search(q, K)), 1))
        out["capacity"], out["count"] = live.describe()["capacity"], live.count
    os.remove(path)
    os.rmdir(root)
    for key in [k for k in out if k.endswith("_us")]:
        out[key + "_median"] = round(statistics.median(out[key]), 1)
    return out


def main():
    out_dir = _opt("--out", "profiles/search_filter", str)
    rounds, launches = _opt("--rounds", 7), _opt("--launches", 50)
    sizes = [int(x) for x in _opt("--sizes", "100000,1000000", str).split(",")]
    os.makedirs(out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tile_rows": OS.tile_rows(),
           "kernels": [], "index": []}
    for N in sizes:
        res["kernels"].append(kernels(N, rounds, launches))
        print(json.dumps(res["kernels"][-1]), flush=True)
    for N in sizes:
        res["index"].append(index(N, rounds, launches))
        print(json.dumps(res["index"][-1]), flush=True)
    lines = ["# Live indexes: the filtered scan against the unfiltered scan (scripts/search_filter_measure.py)", "",
             f"Device: {res['device']}, torch {res['torch']}. D = {D}, k = {K}, Q = {Q}, tile = {res['tile_rows']} rows.", "",
             "## Kernels, launch to launch", "",
             f"Device events around {launches} back-to-back (scan, merge) pairs; medians over {rounds} rounds, the variants "
             "interleaved within each round; in brackets the spread (max - min) over the rounds. `scan` is kinds 31 + 32 and "
             "the other columns kind 33 + 32, all of the library that was loaded for this run.", "",
             "| N | scan + merge (us) | all live, no filter | half dead, random rows | half dead, random whole tiles | "
             "half dead, every other tile | tag filter, 1 % pass |", "|---|---|---|---|---|---|---|"]
    for c in res["kernels"]:
        def col(n, c=c):
            return f"{c['us_median'][n]} [{c['us_spread'][n]}] ({c['over_scan'][n]}x)"
        lines.append(f"| {c['N']} | {c['us_median']['scan']} [{c['us_spread']['scan']}] | " +
                     " | ".join(col(n) for n in VARIANTS[1:]) + " |")
    lines += ["", "Findings:", ""]
    for c in res["kernels"]:
        m, sp = c["us_median"], c["us_spread"]
        diff, noise = m["all_live"] - m["scan"], max(sp["all_live"], sp["scan"])
        verdict = ("slower than the unfiltered path by more than the run-to-run spread" if diff > noise else
                   "faster than the unfiltered path by more than the run-to-run spread" if -diff > noise else
                   "within the run-to-run spread of the unfiltered path")
        lines.append(f"* N = {c['N']}: all live without a filter is {verdict} ({diff:+.1f} us, spread {noise} us). Half the rows "
                     f"dead as whole tiles takes {c['over_scan']['half_dead_tiles']}x the unfiltered time (every other tile: "
                     f"{c['over_scan']['half_dead_tiles_alternate']}x, the live tiles then sit on half of the XCDs), half dead at "
                     f"random {c['over_scan']['half_dead_random']}x, the 1 % tag filter {c['over_scan']['tag_1pct']}x.")
    lines += ["", "## The index (host wall time per call, one context)", "",
              "`search`: a never-mutated index (the unfiltered program) against the same file after one `delete` (the "
              f"filtered program), median of {launches} calls per round, interleaved, median over the rounds. `add` of 1 row "
              "stays inside the last tile (device data only); `add` of 256 rows crosses a tile boundary (the programs are "
              "destroyed): the first search after it builds, runs eagerly and captures, the next one replays.", "",
              "| N | search, unfiltered (us) | search, filtered (us) | add 1 row (us) | add 256 rows (us) | first search "
              "after re-capture (us) | the search after it (us) |", "|---|---|---|---|---|---|---|"]
    for c in res["index"]:
        lines.append(f"| {c['N']} | {c['search_unfiltered_us_median']} | {c['search_filtered_us_median']} | {c['add_1_us_median']} | "
                     f"{c['add_256_us_median']} | {c['first_search_after_recapture_us_median']} | {c['next_search_us_median']} |")
    lines += ["", "Raw:", "", "```json", json.dumps(res, indent=1), "```", ""]
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
