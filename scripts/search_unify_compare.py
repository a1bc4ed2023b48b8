#!/usr/bin/env python3
"""The speed table of profiles/search_unify/README.md from four runs of the two measure scripts: two of a parent
build and two of the build under test, taken in the order parent, new, parent, new, each in a fresh process:

    python scripts/search_filter_measure.py --out RUN/filter && python scripts/search_fp8_measure.py --out RUN/fp8

Per row: floor = the larger of the parent's in-run spreads (max - min over the rounds) and the difference of the
two parent medians; limit = the mean of the two parent medians + floor; a row passes when both medians of the
build under test are at or below the limit. Prints the markdown table and exits nonzero when a row fails.

    python scripts/search_unify_compare.py PARENT1 NEW1 PARENT2 NEW2"""
import json
import os
import sys


def rows(run):
    """{(row, kernels): (median us, spread us)} of one run directory."""
    readme = open(os.path.join(run, "filter", "README.md")).read()
    filt = json.loads(readme.split("```json")[1].split("```")[0])
    fp8 = json.load(open(os.path.join(run, "fp8", "search_fp8.json")))
    out = {}
    for c in filt["kernels"]:
        for v in c["us_median"]:
            out[(f"filter script, N = {c['N']}, Q = 1", v)] = (c["us_median"][v], c["us_spread"][v])
    for c in fp8["speed"]:
        name = f"fp8 script, N = {c['N']}, Q = {c['Q']}" + (", tag 1 %" if c["tag_filter_1pct"] else "")
        for v, kern in (("bf16", "fscan"), ("fp8", "qscan")):
            out[(name, kern)] = (c["us_median"][v], c["us_spread"][v])
    return out


def main():
    p1, n1, p2, n2 = (rows(d) for d in sys.argv[1:5])
    print("| row | kernels | parent 1 | new 1 | parent 2 | new 2 | floor | limit | verdict |")
    print("|---|---|---|---|---|---|---|---|---|")
    failed = 0
    for k in p1:
        floor = max(p1[k][1], p2[k][1], abs(p1[k][0] - p2[k][0]))
        limit = (p1[k][0] + p2[k][0]) / 2 + floor
        ok = n1[k][0] <= limit and n2[k][0] <= limit
        failed += not ok
        cells = " | ".join(f"{m} [{s}]" for m, s in (p1[k], n1[k], p2[k], n2[k]))
        print(f"| {k[0]} | {k[1]} | {cells} | {floor:.1f} | {limit:.1f} | {'pass' if ok else 'FAIL'} |")
    print(f"\n{len(p1) - failed} of {len(p1)} rows pass.")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
