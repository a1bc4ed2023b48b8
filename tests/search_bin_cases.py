"""The oracle and the fixtures of the binary-index tests (numpy only), shared by tests/test_search_bin_cpu.py,
tests/test_search_bin_gpu.py and tests/test_search_bin_index_gpu.py.

Stage-one scores are integers, ``D - 2 * popcount(q xor r)``, so every comparison with the kernel is bit for bit:
no error bound exists. The order rule (higher score first, then the lower id) decides the many ties."""
import numpy as np

T = 256  # HZ_SEARCH_TILE


def binarize(v):
    """fp32 [N, D] -> uint32 [N, D / 32], one column at a time: bit i & 31 of word i >> 5 is 1 iff the sign bit of
    column i is clear (a plain loop over the columns, independent of hipzap.search.binarize's packbits)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    n, d = u.shape
    out = np.zeros((n, d // 32), np.uint32)
    for i in range(d):
        out[:, i >> 5] |= ((u[:, i] >> np.uint32(31)) ^ np.uint32(1)) << np.uint32(i & 31)
    return out


def popcount(x):
    x = np.ascontiguousarray(x, np.uint32).astype(np.uint64)
    c = np.zeros(x.shape, np.int64)
    for _ in range(32):
        c += (x & np.uint64(1)).astype(np.int64)
        x = x >> np.uint64(1)
    return c


def scores(words, qbits):
    """Exact integer scores int64 [Q, N]."""
    d = 32 * words.shape[1]
    return np.stack([d - 2 * popcount(words ^ q[None, :]).sum(axis=1) for q in qbits])


def orderable(f):
    """The kernels' order-preserving u32 of an fp32 score (uint64 array)."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000)


def bin_scan_ref(words, qbits, k, allow=None):
    """The exact keys of the search, uint64 [Q, k] (0 in the slots past the passing rows): ``orderable(score) << 32
    | ~id`` of the passing rows' best k, scores as integers, ties by the lower id. ``allow``: bool [N] or [Q, N]."""
    s = scores(words, qbits)
    n = words.shape[0]
    out = np.zeros((qbits.shape[0], k), np.uint64)
    for q in range(qbits.shape[0]):
        ok = np.ones(n, bool) if allow is None else np.asarray(allow, bool) if np.ndim(allow) == 1 else np.asarray(allow[q], bool)
        ids = np.flatnonzero(ok)
        order = ids[np.lexsort((ids, -s[q, ids]))][:k]
        key = (orderable(s[q, order].astype(np.float32)) << np.uint64(32)) | (order.astype(np.uint64) ^ np.uint64(0xFFFFFFFF))
        out[q, :order.size] = key
    return out


def keys_of(sc, ids):
    """(scores fp32 [Q, k], ids int32 [Q, k]) as the merge writes them -> keys uint64 [Q, k] (0 for -inf / -1)."""
    key = (orderable(np.where(ids >= 0, sc, 0).astype(np.float32)) << np.uint64(32)) | \
        (ids.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)) ^ np.uint64(0xFFFFFFFF)
    return np.where(ids >= 0, key, np.uint64(0))


def make(N, D, Q, seed):
    """-> (row words uint32 [N, D / 32], queries fp32 [Q, D]): random signs; a third of the rows are copies of
    earlier rows and each query is a noisy copy of a row, so ties and near rows are frequent."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, D)).astype(np.float32)
    dup = rng.random(N) < 0.33
    src = (rng.random(N) * np.arange(N)).astype(np.int64)
    v[dup] = v[src[dup]]
    q = v[rng.integers(0, N, Q)] + np.float32(0.8) * rng.standard_normal((Q, D)).astype(np.float32)
    return binarize(v), np.ascontiguousarray(q, np.float32)


# the grid: every D of {128, 256, 768, 1920, 2048} (W = 4, the bucket edge 8, 24, 60, 64), N of {1, 255, 256, 257,
# 700}, Q of {1, 3, 16} and k of {1, 10, 128} appears; both row pitches run for every case
GRID = [
    # name, N, D, Q, k
    ("n1_d128", 1, 128, 1, 1),
    ("n255_d256", 255, 256, 3, 10),
    ("n256_d768", 256, 768, 16, 10),
    ("n257_d1920", 257, 1920, 3, 128),
    ("n700_d2048", 700, 2048, 16, 128),
    ("n700_d128_k1", 700, 128, 16, 1),
    ("n257_d768_q1", 257, 768, 1, 128),
    ("n700_d256", 700, 256, 1, 10),
    ("n255_d2048", 255, 2048, 3, 1),
    ("n256_d1920", 256, 1920, 16, 10),
]
GRID_NAMES = [g[0] for g in GRID]


def grid_case(name):
    for i, (n, N, D, Q, k) in enumerate(GRID):
        if n == name:
            words, q = make(N, D, Q, 100 + i)
            return words, q, k
    raise KeyError(name)


def live_pattern(name, N):
    r = np.arange(N)
    if name == "all":
        return np.ones(N, bool)
    if name == "wave_dead":     # rows 64..127 of every tile: one wave's rows all fail
        return (r % T) // 64 != 1
    if name == "tile_dead":     # the second tile is dead whole
        return r // T != 1
    if name == "alternating":
        return r % 2 == 0
    raise KeyError(name)


LIVE_PATTERNS = ("all", "wave_dead", "tile_dead", "alternating")


# ------------------------------------------------------------------------ index-level fixtures
def sign_edge_values():
    """fp32 values whose sign bit is all that matters: zeros, the smallest subnormals of fp32 and of bf16 of either
    sign, values that round to zero magnitude in bf16, and ordinary values."""
    tiny32 = np.array([1], np.uint32).view(np.float32)[0]          # 2^-149
    tiny16 = np.array([0x00010000], np.uint32).view(np.float32)[0]  # the smallest bf16 subnormal
    half16 = np.array([0x00008000], np.uint32).view(np.float32)[0]  # a tie: rounds to zero magnitude (even)
    below = np.array([0x00007FFF], np.uint32).view(np.float32)[0]   # rounds to zero magnitude
    vals = [0.0, -0.0, tiny32, -tiny32, tiny16, -tiny16, half16, -half16, below, -below, 1.0, -1.0, 3.5e-3, -3.5e-3]
    return np.array(vals, np.float32)


def clusters(D, nclust=4, per=90, seed=7, spread=0.05):
    """A few tight clusters of at most 100 rows (fp32 [nclust * per, D]) and one query near each centre: inside a
    cluster every row has nearly the same sign pattern, so the sign bits cannot order it, while the Hamming top 128
    under the order rule holds the whole cluster -- and with it every bf16 top-10 id."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nclust, D)).astype(np.float32)
    v = np.repeat(cent, per, axis=0) + np.float32(spread) * rng.standard_normal((nclust * per, D)).astype(np.float32)
    q = cent + np.float32(spread) * rng.standard_normal((nclust, D)).astype(np.float32)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(q, np.float32)


IX_N = 300  # the live scenario's first index: it ends inside its second tile


def index_data(D, seed=11):
    """A [IX_N, D], B [T, D] (its rows cross a tile boundary and the capacity when added) and queries [3, D]."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((IX_N + T, D)).astype(np.float32)
    q = v[rng.integers(0, IX_N, 3)] + np.float32(0.5) * rng.standard_normal((3, D)).astype(np.float32)
    return v[:IX_N].copy(), v[IX_N:].copy(), np.ascontiguousarray(q, np.float32)
