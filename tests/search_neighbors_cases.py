"""The cases of the neighbour-search tests (HZ_K_SEARCH_MSCAN / HZ_K_SEARCH_MERGEN, ``Index.neighbors``), shared by
tests/test_search_neighbors_cpu.py -- which asserts from the fp64 oracle alone how many queries of each case have a
forced answer -- and the two GPU files.

Bound: every product of two bf16 values is exact in fp32, and a score is D fp32 additions inside and between MFMAs
whose internal rounding is not documented as round-to-nearest. ``beta(D) * sum_i |a_i b_i|`` with ``beta(D) =
D * 2^-23 / (1 - D * 2^-23)`` holds for any order of the additions and for truncating adds; it is twice the
``gamma`` of tests/test_search_gpu.py. "Forced" is that file's ``ambiguous`` criterion evaluated with ``beta``."""
import numpy as np

from hipzap import search as S

from test_search_gpu import T, ambiguous, make  # noqa: F401  (re-exported)

QB = 64  # HZ_SEARCH_SELF_QB


def beta(D):
    return D * 2.0 ** -23 / (1 - D * 2.0 ** -23)


def live_pattern(name, N):
    """bool [N]: which rows are live."""
    live = np.ones(N, bool)
    if name == "all":
        pass
    elif name == "one_dead":
        live[N // 2] = False
    elif name == "dead_group":  # a whole group of 16 rows (one MFMA operand), and half of the next one
        live[32:48] = False
        live[48:56] = False
    elif name == "dead_tile":  # the whole second tile, and one row of the last, partial one
        live[T:2 * T] = False
        live[N - 2] = False
    elif name == "alternating":
        live[1::2] = False
    else:
        raise KeyError(name)
    return live


def pick_ids(N, Q, live, seed):
    """Q ids of live rows in a scrambled order: the first and the last live row, one id twice, the rest drawn with
    replacement where Q exceeds the live rows."""
    rng = np.random.default_rng(1000 + seed)
    rows = np.flatnonzero(live)
    ids = rng.choice(rows, Q, replace=Q > rows.size)
    if Q >= 2:
        ids[0], ids[-1] = rows[-1], rows[0]
    if Q >= 4:
        ids[2] = ids[1]  # a repeated id
    return ids.astype(np.int32)


# (name, N, D, Q, k, kind, live pattern, skip_self, seed): every N of {1, k, T-1, T, T+1, 3T+5}, D of {32, 96, 768,
# 2048}, Q of {1, QB-1, QB, QB+1, 2QB+3} and k of {1, 10, 128} appears, skip_self both ways
CASES = [
    ("n1", 1, 32, 1, 1, "normal", "all", 0, 0),
    ("n1_skip", 1, 32, 1, 1, "normal", "all", 1, 0),
    ("n_k", 10, 96, QB - 1, 10, "normal", "all", 1, 0),
    ("n_k_self", 10, 96, QB, 10, "normal", "all", 0, 0),
    ("t_m1", T - 1, 768, QB, 10, "normal", "one_dead", 1, 0),
    ("t_group", T, 96, QB + 1, 1, "normal", "dead_group", 0, 0),
    ("t_p1_d2048", T + 1, 2048, 2 * QB + 3, 10, "pos", "all", 1, 0),
    ("t3_tile", 3 * T + 5, 768, 2 * QB + 3, 10, "normal", "dead_tile", 1, 0),
    ("t3_k128", 3 * T + 5, 2048, QB + 1, 128, "pos", "dead_group", 1, 0),
    ("t3_d32_k128", 3 * T + 5, 32, 1, 128, "pos", "one_dead", 0, 0),
    ("t3_neg", 2 * T + 3, 96, QB - 1, 10, "neg", "alternating", 1, 0),
    ("t3_d768_k1", 3 * T + 5, 768, QB - 1, 1, "pos", "dead_tile", 0, 0),
]
NAMES = [c[0] for c in CASES]


def build_case(name):
    """-> (bf16 bits [N, D], the rows as fp32, qid int32 [Q], k, live bool [N], skip_self, kind)."""
    for n, N, D, Q, k, kind, pattern, skip, seed in CASES:
        if n == name:
            bits, c32, _ = make(N, D, 1, seed, kind)
            live = live_pattern(pattern, N)
            return bits, c32, pick_ids(N, Q, live, seed), k, live, skip, kind
    raise KeyError(name)


def allow_of(live, qid, skip_self):
    """bool [Q, N]: the rows each query may return."""
    allow = np.repeat(np.asarray(live, bool)[None, :], len(qid), axis=0)
    if skip_self:
        allow[np.arange(len(qid)), qid] = False
    return allow


_ORACLE = {}


def oracle(c32, qid, k, live, skip_self, key=None):
    """(fp64 scores [Q, N], bounds [Q, N], allow [Q, N], ref scores [Q, k], ref ids [Q, k]); cached under ``key``."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    c64 = c32.astype(np.float64)
    s = np.stack([(c64 * c64[i][None, :]).sum(axis=1) for i in qid])
    b = beta(c32.shape[1]) * np.stack([np.abs(c64 * c64[i][None, :]).sum(axis=1) for i in qid])
    allow = allow_of(live, qid, skip_self)
    rs, ri = S.search_ref(c32, c32[qid], k, allow)
    out = (s, b, allow, rs, ri)
    if key is not None:
        _ORACLE[key] = out
    return out


def case_oracle(name):
    bits, c32, qid, k, live, skip, kind = build_case(name)
    return oracle(c32, qid, k, live, skip, key=name)


def forced(s, b, k, allow, allow_ties=False):
    """bool [Q]: the queries whose answer is forced -- ``ambiguous`` over the query's allowed rows finds nothing."""
    out = np.zeros(s.shape[0], bool)
    for qi in range(s.shape[0]):
        rows = np.flatnonzero(allow[qi])
        out[qi] = rows.size == 0 or ambiguous(s[qi:qi + 1, rows], b[qi:qi + 1, rows], k, allow_ties) == 0
    return out


def check_against_oracle(sc, ids, s, b, allow, rs, ri, k, must=None):
    """The comparison of the issue: for every query the score at each rank lies within the bound of the oracle's score
    at that rank (where an unforced answer holds another row there: within the largest bound of the query's allowed
    rows, which is what bounded errors can move a sorted list's j-th entry by); every returned pair is also within its
    own bound of its own fp64 dot; ids equal the oracle's for the forced queries. -> (forced queries, worst |err| / bound over the returned pairs)."""
    ok = forced(s, b, k, allow) if must is None else must
    worst = 0.0
    for qi in range(s.shape[0]):
        n = int(min(k, allow[qi].sum()))
        bmax = b[qi][allow[qi]].max() if n else 0.0
        assert (ids[qi, n:] == -1).all() and (sc[qi, n:] == -np.inf).all(), (qi, ids[qi], n)
        assert (ids[qi, :n] >= 0).all() and allow[qi][ids[qi, :n]].all(), (qi, ids[qi])
        assert len(set(ids[qi, :n].tolist())) == n, (qi, ids[qi])
        for j in range(n):
            i, r = int(ids[qi, j]), int(ri[qi, j])
            err = abs(float(sc[qi, j]) - s[qi, i])  # the returned pair against its own fp64 dot
            worst = max(worst, err / b[qi, i]) if b[qi, i] > 0 else worst
            assert err <= b[qi, i], (qi, j, i, sc[qi, j], s[qi, i], b[qi, i])
            assert abs(float(sc[qi, j]) - rs[qi, j]) <= (b[qi, r] if i == r else bmax), (qi, j, i, r, sc[qi, j], rs[qi, j])
        if ok[qi]:
            assert np.array_equal(ids[qi], ri[qi]), (qi, ids[qi], ri[qi])
    return ok, worst


def planted_pair(N=3 * T + 5, D=96, seed=5):
    """A "normal" corpus whose rows ``a`` (in tile 0) and ``b`` (in the last, partial tile) hold the same bits
    -> (bits, c32, a, b)."""
    bits, c32, _ = make(N, D, 1, seed)
    a, b = 7, N - 3
    bits[b] = bits[a]
    return bits, S.bf16_to_f32(bits), a, b


# ------------------------------------------------------------------------ the index-level scenario
IX_D, IX_N, IX_SEED = 96, 2 * T - 40, 39


def index_data():
    """A (bf16-exact fp32 [IX_N, D]) and B ([T, D]: its rows cross a tile boundary, then the capacity, when added):
    the "pos" kind under the inner-product metric, every answer forced."""
    bits, c32, _ = make(IX_N + T, IX_D, 1, IX_SEED, "pos")
    return c32[:IX_N].copy(), c32[IX_N:].copy()


def index_ids(n, count):
    """n ids over [0, count): scrambled, the first and the last row among them."""
    ids = np.random.default_rng(77).permutation(count)[:n].astype(np.int32)
    ids[0], ids[-1] = count - 1, 0
    return ids
