"""The cases of the IVF tests, shared by tests/test_search_ivf_cpu.py (which asserts on the host that every
index-level query is forced), tests/test_search_ivf_gpu.py (the list-scan kernel through its launcher) and
tests/test_search_ivf_index_gpu.py (the GPU index)."""
import numpy as np

from hipzap import search as S

from search_filter_cases import T, ambiguous, gamma, make, oracle  # noqa: F401  (re-exported)

# ------------------------------------------------------------------------------ the kernel-level layout
# 7 tiles, 5 lists of 0, 1, 1, 2 and 3 tiles whose tile ids are NOT adjacent in list_tiles; the last list ends in
# a partial tile (100 rows), so 156 stored rows are padding: dead, and filled with a NaN bit pattern
NTILE, NLIST = 7, 5
LIST_OFF = np.array([0, 0, 1, 2, 4, 7], np.int32)
LIST_TILES = np.array([4, 0, 6, 2, 1, 5, 3], np.int32)
LIST_ROWS = [0, T, T, 2 * T, 2 * T + 100]
N_EXT = sum(LIST_ROWS)
NAN_BITS = 0x7FC0
DUP = (40, 1201)  # two ids that hold the same row, in lists 1 and 4: a tie that only the id settles

# (name, D, Q, k, nprobe, user filter): every D of {8, 520, 768, 2048} (NC 1..4, lanes past a row's end), Q of
# {1, 3, 16}, k of {1, 10, 128} and nprobe of {1, 2, 5} appears
KCASES = [
    ("d8_q1_k1_p1", 8, 1, 1, 1, False),
    ("d8_q16_k10_p2", 8, 16, 10, 2, False),
    ("d520_q3_k128_p5", 520, 3, 128, 5, False),
    ("d520_q16_k1_p2", 520, 16, 1, 2, True),
    ("d768_q3_k10_p1", 768, 3, 10, 1, True),
    ("d768_q1_k128_p2", 768, 1, 128, 2, False),
    ("d2048_q16_k10_p5", 2048, 16, 10, 5, False),
    ("d2048_q3_k128_p1", 2048, 3, 128, 1, True),
]
KNAMES = [c[0] for c in KCASES]


def kernel_layout(D, Q, seed=31):
    """-> dict: ``bits`` (the stored rows, uint16 [7 T, D], NaN patterns on padding), ``rowid`` int32 [7 T],
    ``live`` bool [7 T], ``tags`` uint32 [7 T] (bit l for list l, the user's tag from bit 8 up), ``list_of``
    (the list of each stored row, -1 on padding), ``q`` fp32 [Q, D], ``ext`` (the rows by id, uint16 [N_EXT, D])."""
    ext, _, q = make(N_EXT, D, Q, seed)
    ext[DUP[0]] = ext[DUP[1]] = S.to_bf16((q[0] * np.float32(2.5))[None, :])[0]  # well above the N(0, 1) rows
    rng = np.random.default_rng(seed)
    perm = rng.permutation(N_EXT)
    perm = perm[(perm != DUP[0]) & (perm != DUP[1])]
    bits = np.full((NTILE * T, D), NAN_BITS, np.uint16)
    rowid = np.full(NTILE * T, -1, np.int32)
    list_of = np.full(NTILE * T, -1, np.int32)
    at = 0
    for l in range(NLIST):
        n = LIST_ROWS[l]
        take = n - (l in (1, 4))
        ids = list(perm[at:at + take])
        at += take
        if l == 1:
            ids.append(DUP[0])
        if l == 4:
            ids.append(DUP[1])
        ids = np.sort(np.array(ids, np.int64))  # ascending inside a list
        tiles = LIST_TILES[LIST_OFF[l]:LIST_OFF[l + 1]]
        pos = (tiles[:, None].astype(np.int64) * T + np.arange(T)[None, :]).reshape(-1)[:n]
        rowid[pos], bits[pos], list_of[pos] = ids, ext[ids], l
    live = rowid >= 0
    user = (np.where(live, rowid, 0) % 3).astype(np.uint32)
    tags = np.where(live, (1 << np.maximum(list_of, 0)).astype(np.uint32) | (user << 8), 0).astype(np.uint32)
    return {"bits": bits, "rowid": rowid, "live": live, "tags": tags, "list_of": list_of, "q": q, "ext": ext}


def kernel_probes(Q, nprobe, seed=5):
    """int32 [Q, nprobe]: distinct lists per query, in an order of their own; query 0 probes lists 1 and 4 first
    when it can (the duplicate pair), and some query probes the empty list 0."""
    rng = np.random.default_rng(seed + 7 * nprobe)
    out = np.stack([rng.permutation(NLIST)[:nprobe] for _ in range(Q)]).astype(np.int32)
    if nprobe >= 2:
        out[0, :2] = (4, 1)
        for j in range(2, nprobe):
            out[0, j] = [l for l in range(NLIST) if l not in out[0, :j]][0]
    if Q > 1 and nprobe == 1:
        out[1, 0] = 0  # a probe set without a tile
    return out


def probe_tiles(probes):
    """The tiles each query's probe set holds, in probe order: list of int arrays."""
    return [np.concatenate([LIST_TILES[LIST_OFF[l]:LIST_OFF[l + 1]] for l in row] + [np.zeros(0, np.int32)]) for row in probes]


# ------------------------------------------------------------------------------ the index-level scenario
# the seed makes every query forced at nprobe 1 and 2, k 1 and 10 (asserted in tests/test_search_ivf_cpu.py)
IX_N, IX_D, IX_LISTS, IX_Q, IX_SEED = 600, 64, 6, 8, 4


def clustered_data(n=IX_N, d=IX_D, nclus=IX_LISTS, nq=IX_Q, seed=IX_SEED, spread=0.35):
    """``n`` vectors around ``nclus`` random directions and ``nq`` queries near some of the vectors, fp32."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nclus, d))
    v = cent[rng.integers(0, nclus, n)] + spread * rng.standard_normal((n, d))
    q = v[rng.choice(n, nq, replace=False)] + 0.5 * spread * rng.standard_normal((nq, d))
    return v.astype(np.float32), S.normalize_rows(q.astype(np.float32))


def index_tags(n=IX_N):
    return ((np.arange(n) * 7) % 5).astype(np.uint32)


def forced(ref, q, k, nprobe, allow=None):
    """The host criterion that the IVF answer of ``ref`` (a RefIndex of an IVF file) for queries ``q`` is
    determined: the gap between the nprobe-th and the next centroid score is above twice the ``gamma`` bound of
    both, and the top k over the rows of the probed lists (and of ``allow``, bool [N]) is unambiguous under
    ``ambiguous``. -> bool [Q]."""
    q = np.asarray(q, np.float32)
    nlist = ref.ivf["nlist"]
    cs, cb, _, _ = oracle(ref._cent, q, min(nprobe, nlist))
    s, b, _, _ = oracle(ref._rows, q, k)
    out = np.ones(q.shape[0], bool)
    for qi in range(q.shape[0]):
        near = np.ones(ref.count, bool)
        if nprobe < nlist:
            order = np.argsort(-cs[qi], kind="stable")
            srt, bs = cs[qi][order], cb[qi][order]
            close = srt[:-1] - srt[1:] <= 2 * np.maximum(bs[:-1], bs[1:])
            if close[:nprobe].any():  # the probes' own order and the boundary after them
                out[qi] = False
            near = np.isin(ref.ivf["list_of"], order[:nprobe])
        rows = np.flatnonzero(near & ref._live & (True if allow is None else allow))
        if rows.size and ambiguous(s[qi:qi + 1, rows], b[qi:qi + 1, rows], k):
            out[qi] = False
    return out
