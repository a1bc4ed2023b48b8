"""The cases of the fp8-index tests, shared by tests/test_search_fp8_cpu.py (which asserts on the host that every
case is unambiguous over its passing rows) and the two GPU files tests/test_search_fp8_gpu.py and
tests/test_search_fp8_index_gpu.py.

Bound: the kernel's score is one fp32 product applied to a D-term fp32 sum, so
``|gpu - fp64| <= gamma(D + 1) * |scale_r| * sum_i |q_i c_ri|`` with the suite's ``gamma``."""
import numpy as np

from hipzap import search as S

import search_filter_cases as F
from search_filter_cases import T, ambiguous, gamma, make  # noqa: F401  (re-exported)


def make_q(N, D, Q, seed, kind="normal"):
    """-> (codes uint8 [N, D], scales fp32 [N], queries fp32 [Q, D]): ``make``'s rows through the quantiser."""
    _, c32, q = make(N, D, Q, seed, kind)
    codes, scales = S.quantize_rows(c32)
    return codes, scales, q


def live_pattern(name, N, k):
    if name == "dead_groups":  # every other group of four rows is dead (the kernel skips such a group whole)
        return (np.arange(N) // 4) % 2 == 0
    return F.live_pattern(name, N, k)


def oracle_q(codes, scales, q):
    """(fp64 scores [Q, N], bounds [Q, N]) of the decoded rows times their scales."""
    c64, q64, s64 = S.e4m3_to_f32(codes).astype(np.float64), q.astype(np.float64), scales.astype(np.float64)
    s = np.stack([(c64 * r[None, :]).sum(axis=1) * s64 for r in q64])
    b = gamma(codes.shape[1] + 1) * np.stack([np.abs(c64 * r[None, :]).sum(axis=1) * np.abs(s64) for r in q64])
    return s, b


def ref_ids(codes, scales, q, k, allow):
    return S.search_ref(S.e4m3_to_f32(codes), q, k, allow, scales=scales)[1]


# (name, N, D, Q, k, kind, live pattern, seed): every N of {1, 9, T-1, T, T+1, 3T+5}, D of {16, 80, 768, 1024, 1040,
# 2048}, Q of {1, 3, 16} and k of {1, 10, 128} appears; the seeds make every case unambiguous over its live rows
CASES = [
    ("n1", 1, 16, 1, 1, "normal", "all", 0),
    ("n9_below_k", 9, 80, 3, 10, "normal", "all", 0),
    ("tm1_groups", T - 1, 768, 1, 10, "normal", "dead_groups", 0),
    ("t_d1024", T, 1024, 16, 10, "pos", "all", 0),
    ("tp1_d1040_k128", T + 1, 1040, 3, 128, "pos", "dead_groups", 0),
    ("dead_tile", 3 * T + 5, 768, 3, 10, "normal", "mid_tile_dead", 0),
    ("few_total", 3 * T + 5, 80, 3, 10, "normal", "few_total", 0),
    ("lds_max", 3 * T + 5, 2048, 16, 10, "pos", "all", 0),
    ("k128", 3 * T + 5, 768, 1, 128, "pos", "all", 0),
    ("d16_k1", 3 * T + 5, 16, 16, 1, "normal", "dead_groups", 0),
    ("neg_partial", 2 * T + 3, 80, 3, 10, "neg", "dead_groups", 0),
]
NAMES = [c[0] for c in CASES]


def build_case(name):
    """-> (codes, scales, queries, k, live bool [N])."""
    for n, N, D, Q, k, kind, pattern, seed in CASES:
        if n == name:
            codes, scales, q = make_q(N, D, Q, seed, kind)
            return codes, scales, q, k, live_pattern(pattern, N, k)
    raise KeyError(name)


# ------------------------------------------------------------------------ the index-level scenarios
IX_D, IX_SEED = 80, 31


def index_data():
    """A [F.IX_N, D], B [T, D] (its rows cross a tile boundary when added) and queries [3, D] for ``F.drive``: the
    "pos" kind, whose scores spread over decades, under the inner-product metric."""
    _, c32, q = make(F.IX_N + T, IX_D, 3, IX_SEED, "pos")
    return c32[:F.IX_N].copy(), c32[F.IX_N:].copy(), q


BIG_N, BIG_D, BIG_SEED = 3 * T + 5, 768, 33


def big_data():
    """fp32 rows [3T+5, 768] ("pos") and 20 queries: the index against RefIndex for Q in {1, 16, 20}."""
    _, c32, q = make(BIG_N, BIG_D, 20, BIG_SEED, "pos")
    return c32, q


def index_unambiguous(ix, q, k, allow=None):
    """Host: the answer of RefIndex ``ix`` (fp8) for ``q`` is forced under twice the bound."""
    s, b = oracle_q(ix._bits, ix.scales, q)
    return F.subset_ambiguous(s, b, k, ix._live if allow is None else allow) == 0
