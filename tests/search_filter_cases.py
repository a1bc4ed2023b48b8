"""The cases of the filtered-search tests, shared by tests/test_search_filter_cpu.py (which asserts on the
host that every case is unambiguous over its passing rows) and tests/test_search_filter_gpu.py."""
import numpy as np

from hipzap import search as S

from test_search_gpu import T, ambiguous, gamma, make, oracle, plant  # noqa: F401  (re-exported)


def live_pattern(name, N, k):
    """bool [N]: which rows are live."""
    live = np.zeros(N, bool)
    if name == "all":
        live[:] = True
    elif name == "none":
        pass
    elif name == "last_of_partial":  # whole tiles live, the partial tile only its last row
        live[:N // T * T] = True
        live[N - 1] = True
    elif name == "mid_tile_dead":
        live[:] = True
        live[T:2 * T] = False
    elif name == "alternating":
        live[::2] = True
    elif name == "few_per_tile":  # k - 6 live rows in every tile (the partial one included): below k each, above k in all
        for t0 in range(0, N, T):
            rows = min(T, N - t0)
            live[t0 + (np.arange(k - 6) * 37 + 1) % rows] = True
    elif name == "few_total":  # k - 7 live rows in all, in two tiles
        live[[5, T + 9, N - 2][:max(k - 7, 1)]] = True
    else:
        raise KeyError(name)
    return live


# (name, N, D, Q, k, kind, live pattern, seed): every N of {1, T-1, T, T+1, 3T+5}, D of {8, 72, 768, 2048}, Q of
# {1, 3, 16} and k of {1, 10, 128} appears; the seeds make every case unambiguous over its live rows
CASES = [
    ("all_n1", 1, 8, 1, 1, "normal", "all", 0),
    ("none_tm1", T - 1, 72, 3, 10, "normal", "none", 0),
    ("alt_t", T, 768, 16, 10, "pos", "alternating", 0),
    ("alt_tp1_k128", T + 1, 2048, 3, 128, "pos", "alternating", 0),
    ("last_of_partial", 3 * T + 5, 72, 1, 10, "normal", "last_of_partial", 0),
    ("mid_tile_dead", 3 * T + 5, 768, 3, 10, "normal", "mid_tile_dead", 0),
    ("few_per_tile", 3 * T + 5, 8, 16, 10, "normal", "few_per_tile", 0),
    ("few_total", 3 * T + 5, 72, 3, 10, "normal", "few_total", 0),
    ("all_k1", 3 * T + 5, 2048, 16, 1, "pos", "all", 0),
    ("all_k128", 3 * T + 5, 768, 1, 128, "pos", "all", 1),
    ("neg_partial", 2 * T + 3, 72, 3, 10, "neg", "alternating", 0),
]
NAMES = [c[0] for c in CASES]


def build_case(name):
    """-> (bf16 bits [N, D], the rows as fp32, queries, k, live bool [N])."""
    for n, N, D, Q, k, kind, pattern, seed in CASES:
        if n == name:
            bits, c32, q = make(N, D, Q, seed, kind)
            return bits, c32, q, k, live_pattern(pattern, N, k)
    raise KeyError(name)


def allowed_oracle(c32, q, k, allow):
    """The oracle over the allowed rows: (fp64 scores [Q, N], bounds [Q, N], ref ids [Q, k]); ``allow`` [N] or [Q, N]."""
    s, b, _, _ = oracle(c32, q, k)
    return s, b, S.search_ref(c32, q, k, allow)[1]


def subset_ambiguous(s, b, k, allow):
    """``ambiguous`` of the existing suite applied to each query's allowed rows."""
    bad = 0
    for qi in range(s.shape[0]):
        rows = np.flatnonzero(allow if allow.ndim == 1 else allow[qi])
        if rows.size:
            bad += ambiguous(s[qi:qi + 1, rows], b[qi:qi + 1, rows], k)
    return bad


# ------------------------------------------------------------------------ the index-level scenario
IX_D, IX_N, IX_SEED = 72, 2 * T - 40, 21


def index_data():
    """A (bf16-exact fp32 [IX_N, D]), B ([T, D]: its rows cross a tile boundary when added), queries [3, D]: the
    "pos" kind, whose scores spread over decades, under the inner-product metric."""
    bits, c32, q = make(IX_N + T, IX_D, 3, IX_SEED, "pos")
    return c32[:IX_N].copy(), c32[IX_N:].copy(), q


def index_tags(n, first=0):
    return ((np.arange(first, first + n) * 7) % 5).astype(np.uint32)


def drive(ix, B, q):
    """One sequence of calls on an open index (GPU or host) -> the list of (scores, ids) it saw."""
    out = [ix.search(q, 10)]
    ids = ix.add(B[:30], tags=index_tags(30, IX_N))          # inside the last tile
    out.append(ix.search(q, 10))
    ids2 = ix.add(B[30:], tags=index_tags(T - 30, IX_N + 30))  # crosses a tile boundary
    out.append(ix.search(q, 10))
    best = int(out[-1][1][0, 0])
    assert ix.delete([best, int(ids[3])]) == 2 and ix.delete([best]) == 0
    out.append(ix.search(q, 10))
    out.append(ix.search(q, 10, filter=(0xFFFFFFFF, 3)))
    out.append(ix.search(q, 7, filter=[(0, 0), (0xFFFFFFFF, 9), (1, 1)]))  # all, none (no tag is 9), odd tags
    ix.set_tags([int(ids2[0]), 4], [9, 9])
    out.append(ix.search(q, 7, filter=[(0, 0), (0xFFFFFFFF, 9), (1, 1)]))
    return out
