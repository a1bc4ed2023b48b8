"""The cases of the two-stage search tests (fp8 scan, exact bf16 rescoring of the candidates), shared by
tests/test_search_rescore_cpu.py (which asserts on the host that the index-level answers are forced) and the GPU
files tests/test_search_rescore_gpu.py and tests/test_search_rescore_index_gpu.py.

When is a two-stage answer forced? Stage two only orders what stage one hands it, so (a) every member of the bf16
oracle's top k must stand inside the fp8 oracle's top R by more than twice the largest ``oracle_q`` bound of the
query (then the GPU's stage one, whose scores lie within that bound of the fp8 oracle's, hands it over), and (b)
the bf16 top k must be unambiguous under the suite's criterion (``ambiguous`` of tests/test_search_gpu.py). Where R
covers every passing row, (a) holds trivially and the second stage's answer is the bf16 index's, bit for bit."""
import numpy as np

from hipzap import search as S

import search_fp8_cases as P
from search_filter_cases import T, ambiguous, gamma, make, oracle  # noqa: F401  (re-exported)

MAX_K = 128

# ------------------------------------------------------------------------------------ kernel level
BITS_N = 300                       # two tiles, one partial
BITS_D = (8, 520, 768, 1544, 2048)  # NC 1 .. 4, lanes past a row's end (520, 1544), full rows
BITS_Q = (1, 3, 16)


def bits_corpus(D, seed=50):
    """-> (bf16 bits [BITS_N, D], the rows as fp32, 16 queries): N(0, 1)."""
    return make(BITS_N, D, 16, seed + D)


def choose_ids(Q, N, R=MAX_K, real=100, seed=0):
    """int32 [Q, R]: per query a shuffled choice of ``real`` distinct ids of [0, N) with R - real slots of -1 mixed in."""
    rng = np.random.default_rng(seed)
    out = np.full((Q, R), -1, np.int32)
    for q in range(Q):
        out[q, :real] = rng.choice(N, real, replace=False)
        out[q] = out[q][rng.permutation(R)]
    return out


# ------------------------------------------------------------------------------------ index level
IX_N, IX_D = 600, 64  # three tiles: stage-one candidates come from more than two tile lists


def covered_data(seed=60):
    """N(0, 1) vectors [IX_N, IX_D], tags of which exactly 120 rows pass ``(0xFFFFFFFF, 1)``, and 3 queries."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((IX_N, IX_D)).astype(np.float32)
    tags = np.zeros(IX_N, np.uint32)
    tags[rng.choice(IX_N, 120, replace=False)] = 1
    return v, tags, rng.standard_normal((3, IX_D)).astype(np.float32)


COVER_FILTER = (0xFFFFFFFF, 1)


def covered_deletes(seed=61):
    """The 500 ids whose deletion leaves 100 live rows."""
    return np.sort(np.random.default_rng(seed).choice(IX_N, IX_N - 100, replace=False)).astype(np.int32)


CLUSTER_SEED, CLUSTERS, SIGMA = 70, 6, 0.05


def clustered_data(seed=CLUSTER_SEED):
    """6 clusters of 100 rows around random unit centres (sigma 0.05 per coordinate) and 3 queries, each a fresh
    point of one cluster: inside a cluster the fp8 score error (about 2e-3) is above the distance between
    neighbouring scores, so the fp8 order of a cluster is not the bf16 one, while the cluster itself is found."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((CLUSTERS, IX_D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    member = np.repeat(np.arange(CLUSTERS), IX_N // CLUSTERS)
    v = centres[member] + SIGMA * rng.standard_normal((IX_N, IX_D))
    q = centres[[0, 3, 5]] + SIGMA * rng.standard_normal((3, IX_D))
    return v.astype(np.float32), S.normalize_rows(q.astype(np.float32))


def write_pair(tmp, v, metric="cosine", tags=None, name="ix"):
    """The version-4, version-3 and bf16 files of the same vectors -> their paths."""
    p4, p3, p1 = (str(tmp / f"{name}{s}.hzidx") for s in ("4", "3", "1"))
    S.write_index(p4, v, metric, tags=tags, dtype="fp8", rescore=True)
    S.write_index(p3, v, metric, tags=tags, dtype="fp8")
    S.write_index(p1, v, metric, tags=tags)
    return p4, p3, p1


def forced(ref, q, k, R=MAX_K, filt=None):
    """Host: is the two-stage answer of RefIndex ``ref`` (version 4) for ``q`` forced? (a) and (b) of the module text."""
    allow = ref.allow(None if filt is None else S.check_filter(filt, q.shape[0]))
    s8, b8 = P.oracle_q(ref._bits, ref.scales, q)
    s16, b16, _, _ = oracle(ref._rrows, q, k)
    for qi in range(q.shape[0]):
        rows = np.flatnonzero(allow if allow.ndim == 1 else allow[qi])
        if ambiguous(s16[qi:qi + 1, rows], b16[qi:qi + 1, rows], k):
            return False
        if rows.size > R:
            order8 = rows[np.argsort(-s8[qi, rows], kind="stable")]
            top16 = rows[np.argsort(-s16[qi, rows], kind="stable")[:k]]
            if not np.all(s8[qi, top16] - s8[qi, order8[R]] > 2 * b8[qi, rows].max()):
                return False
    return True


# the live scenario: "pos" rows (scores spread over decades) under the inner-product metric
LIVE_N0, LIVE_SEED = 200, 80
LIVE_ADDS = (30, 40, 250, 260)  # inside a tile; across the capacity 256 (grow to 512); grow again; across the tile boundary 768 inside the capacity


def live_data():
    _, c32, q = make(LIVE_N0 + sum(LIVE_ADDS), IX_D, 3, LIVE_SEED, "pos")
    return c32, q


def live_tags(n, first=0):
    return ((np.arange(first, first + n) * 7) % 5).astype(np.uint32)


def drive(ix, rows, q, tmp, on_step=None):
    """One sequence of calls on an open version-4 index (GPU or host) -> per step (ids, captured programs before
    the step's search, and after it; None on the host). ``on_step(ix, k, filter)`` runs before each search (the
    CPU test's forcedness check). Ends with a save to ``tmp``."""
    out = []

    def see(k=10, filt=None):
        if on_step:
            on_step(ix, k, filt)
        before = ix.describe().get("programs")  # after the mutation, before the search re-captures
        ids = ix.search(q, k, filter=filt, refine=MAX_K)[1]
        out.append((ids, before, ix.describe().get("programs")))
    see()
    at = LIVE_N0
    for n in LIVE_ADDS:
        ix.add(rows[at:at + n], tags=live_tags(n, at))
        at += n
        see()
    best = int(out[-1][0][0, 0])
    assert ix.delete([best, 7]) == 2
    see()
    see(7, (0xFFFFFFFF, 3))
    ix.set_tags([best + 1 if best + 1 < at else 0, 9], [3, 3])
    see(7, (0xFFFFFFFF, 3))
    ix.save(str(tmp))
    return out
