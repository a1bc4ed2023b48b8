"""The cases of the IVF bulk-search tests, shared by tests/test_search_batch_ivf_cpu.py (``RefIndex`` and
the claims about these inputs) and tests/test_search_batch_ivf_gpu.py (the GPU index and the kernels).

The corpus: 700 rows in 5 lists around the axes e_0 .. e_4, the centroids given (``ivf_init``, no k-means round): list 0
holds 300 rows (two tiles), list 1 holds 10 (fewer than a 16-row group), list 2 is EMPTY, lists 3 and 4 hold 200 and
190. Ids are a permutation, so low ids lie in every list. The 70 queries: 66 aimed at list 0 (two work items per tile,
the second with 2 queries), one alone at list 1, and one each at lists 2, 3 and 4; every query's second choice is list
3 or 4, so nobody but query 66 probes list 1 at nprobe 1 or 2."""
import numpy as np

from hipzap import search as S

NLIST, SIZES = 5, (300, 10, 0, 200, 190)
N, Q = sum(SIZES), 70
DIMS = (32, 96, 128)
LONE = 66          # the query that probes list 1
EMPTY = 67         # the query whose first list is the empty list 2
CENT_SCALE = (1.0, 2.0, 0.5, 1.5, 1.25)  # the ``ip`` index: centroids of unequal norms


def data(d, metric, seed=11):
    """-> (vectors fp32 [N, d], list of each id, init centroids fp32 [5, d], queries fp32 [Q, d])."""
    rng = np.random.default_rng(seed + d)
    list_of = np.repeat(np.arange(NLIST), SIZES)[rng.permutation(N)]
    v = (0.25 / np.sqrt(d)) * rng.standard_normal((N, d)).astype(np.float32)
    v[np.arange(N), list_of] += 1.0
    init = np.zeros((NLIST, d), np.float32)
    init[np.arange(NLIST), np.arange(NLIST)] = 1.0 if metric == "cosine" else np.array(CENT_SCALE, np.float32)
    aim = np.array([0] * 66 + [1, 2, 3, 4])
    q = (0.25 / np.sqrt(d)) * rng.standard_normal((Q, d)).astype(np.float32)
    q[:, :NLIST] = -0.2
    q[np.arange(Q), aim] = 1.0
    second = np.where(aim == 3, 4, np.where((aim == 4) | (np.arange(Q) % 2 == 0), 3, 4))
    q[np.arange(Q), second] = 0.5
    return v.astype(np.float32), list_of, init, q.astype(np.float32)


def write(path, d, metric="cosine"):
    v, list_of, init, q = data(d, metric)
    S.write_index(path, v, metric, ivf=NLIST, nprobe=2, ivf_iters=0, ivf_init=init)
    assert np.array_equal(S.read_ivf(path)["list_of"], list_of)  # the lists are the ones described above
    return q


def probed_rows(ref, q, lists):
    """bool [Q, N]: the live rows each query may return at ``lists`` probes (0: every list), from the host index."""
    live = np.broadcast_to(ref._live, (q.shape[0], ref._live.size))
    if not lists:
        return live
    return live & (ref.ivf["list_of"][None, :, None] == ref.probes(q, lists)[:, None, :]).any(axis=2)


def clauses(ref, q, k, lists, candidates):
    """Which clause of the certificate can certify each query: (fewer than R live rows probed, at least R)."""
    few = probed_rows(ref, q, lists).sum(axis=1) < S.batch_candidates(k, candidates)
    return few, ~few


def forced(ref, q, k, lists):
    """The fp64 oracle over the probed live rows -> (ids [Q, k], bool [Q]: every gap down to rank k + 1 exceeds twice the
    slack, so rounding cannot reorder the answer)."""
    s, i = S.search_ref(ref._rows, q, k + 1, probed_rows(ref, q, lists))
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(s[:, 1:]), s[:, :-1] - s[:, 1:], np.inf).min(axis=1)
    return i[:, :k], gap > 2 * S.batch_slack(q, "cosine")
