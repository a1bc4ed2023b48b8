"""The cases of the bulk-search tests (HZ_K_SEARCH_XSCAN / HZ_K_SEARCH_RESCOREN, ``Index.search_batch``), shared by
tests/test_search_batch_cpu.py -- which asserts from the fp64 oracle alone how many (query, slot) pairs of each case
are forced -- and the two GPU files.

Bound (csrc/hipzap.h, the batch scan's CONTRACT): every product of a split term and a bf16 row value is exact in fp32,
and a score is 3D fp32 additions inside and between MFMAs whose rounding is not documented, so against the exact
``sum_i x'_i r_i`` the error is at most ``beta(3D) * sum_i (|h'_i| + |m'_i| + |l'_i|) |r_i|`` with the ``beta`` of
tests/search_neighbors_cases.py. A slot of the oracle's list is "forced" when the ``ambiguous`` criterion of
tests/test_search_gpu.py, evaluated with this bound, finds its score apart from both neighbours in the sorted order."""
import numpy as np

from hipzap import search as S

from search_neighbors_cases import beta, live_pattern
from test_search_gpu import T, gamma, make  # noqa: F401  (re-exported)

QB = 64  # HZ_SEARCH_SELF_QB


def eff64(q):
    """The effective query x' = h' + m' + l' in fp64 (exact), and sum of the terms' magnitudes."""
    h, m, l = (t.astype(np.float64) for t in S.split3(q))
    return h + m + l, np.abs(h) + np.abs(m) + np.abs(l)


# (name, N, D, Q, k, kind, live pattern, seed): every D of {32, 64, 768}, N of {300, 256}, Q of {1, 64, 65, 130} and
# k of {1, 10, 64, 65, 128} appears. "normal" data only where few slots are asked of a low dimension; the "pos" kind
# spreads the scores over decades, so deep lists stay forced under the bound.
CASES = [
    ("d32_q1_k1", 300, 32, 1, 1, "normal", "all", 0),
    ("d64_q64_k10", 256, 64, 64, 10, "normal", "one_dead", 0),
    ("d768_q65_k64", 300, 768, 65, 64, "pos", "dead_group", 0),
    ("d64_q130_k65", 300, 64, 130, 65, "pos", "all", 0),
    ("d32_q65_k128", 300, 32, 65, 128, "pos", "alternating", 0),
    ("d768_q130_k10", 256, 768, 130, 10, "pos", "all", 0),
    ("d64_q1_k128_neg", 300, 64, 1, 128, "neg", "dead_tile", 0),
]
NAMES = [c[0] for c in CASES]
MAX_UNFORCED = 0.02  # the share of (query, slot) pairs that may be unforced, per case


def build_case(name):
    """-> (bf16 bits [N, D], the rows as fp32, queries fp32 [Q, D], k, live bool [N], kind)."""
    for n, N, D, Q, k, kind, pattern, seed in CASES:
        if n == name:
            bits, c32, q = make(N, D, Q, seed, kind)
            return bits, c32, q, k, live_pattern(pattern, N), kind
    raise KeyError(name)


_ORACLE = {}


def oracle(c32, q, k, live, key=None):
    """(fp64 scores of the split queries [Q, N], bounds [Q, N], ref scores [Q, k], ref ids [Q, k], forced bool [Q, k]);
    cached under ``key``. A slot past the live rows is forced (-1 / -inf)."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    c64 = c32.astype(np.float64)
    x, mag = eff64(q)
    s = x @ c64.T
    b = beta(3 * c32.shape[1]) * (mag @ np.abs(c64).T)
    rs, ri = S.search_ref(c32, x, k, live)
    forced = np.ones((q.shape[0], k), bool)
    rows = np.flatnonzero(live)
    for qi in range(q.shape[0]):
        order = rows[np.argsort(-s[qi, rows], kind="stable")]
        srt, bs = s[qi, order], b[qi, order]
        close = srt[:-1] - srt[1:] < 2 * np.maximum(bs[:-1], bs[1:])  # `ambiguous`: neighbours nearer than twice the bound
        near = np.zeros(order.size, bool)  # slot j: too close to the slot before or after it
        near[:-1] |= close
        near[1:] |= close
        n = min(k, order.size)
        forced[qi, :n] = ~(near[:n])
    out = (s, b, rs, ri, forced)
    if key is not None:
        _ORACLE[key] = out
    return out


def case_oracle(name):
    bits, c32, q, k, live, kind = build_case(name)
    return oracle(c32, q, k, live, key=name)


def check_against_oracle(sc, ids, s, b, rs, ri, forced, live):
    """Every returned pair is a live row within its own bound of its own fp64 score; the empty slots are the oracle's;
    the ids equal the oracle's in every forced slot -> the worst |err| / bound."""
    worst = 0.0
    k = ids.shape[1]
    nlive = int(np.asarray(live).sum())
    for qi in range(ids.shape[0]):
        n = min(k, nlive)
        assert (ids[qi, n:] == -1).all() and np.isneginf(sc[qi, n:]).all(), (qi, ids[qi])
        assert (ids[qi, :n] >= 0).all() and live[ids[qi, :n]].all() and len(set(ids[qi, :n].tolist())) == n, (qi, ids[qi])
        for j in range(n):
            i = int(ids[qi, j])
            err = abs(float(sc[qi, j]) - s[qi, i])
            assert err <= b[qi, i], (qi, j, i, sc[qi, j], s[qi, i], b[qi, i])
            worst = max(worst, err / b[qi, i]) if b[qi, i] > 0 else worst
        must = forced[qi]
        assert np.array_equal(ids[qi][must], ri[qi][must]), (qi, ids[qi], ri[qi])
    return worst


# ------------------------------------------------------------------------------------- exact cases
def exact_case(N=300, D=64, Q=65, seed=3):
    """Rows in {-1, 0, 1} and integer queries with 2^16 <= |x| < 2^17 whose three split terms are all non-zero: every
    partial sum of every product is an integer below D * 2^17 = 2^23 in magnitude, so it is exact in fp32 in any order and the
    score must be the integer dot product bit for bit -> (bits, c32, q, dots int64 [Q, N])."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-1, 2, (N, D)).astype(np.float32)
    # bits 16..9 are h, 256 + c has nine significant bits: m takes the upper eight, l the last one (c is odd)
    x = (1 << 16) + (rng.integers(0, 128, (Q, D)) << 9) + 256 + (rng.integers(0, 128, (Q, D)) * 2 + 1)
    q = (x * rng.choice([-1, 1], (Q, D))).astype(np.float32)
    bits = S.to_bf16(rows)
    dots = q.astype(np.int64) @ rows.astype(np.int64).T
    return bits, S.bf16_to_f32(bits), q, dots


# ------------------------------------------------------------------------------- the index scenario
IX_N, IX_D, IX_Q, IX_SEED = 1000, 64, 100, 51


def clustered(n=IX_N, d=IX_D, nq=IX_Q, seed=IX_SEED, centers=20, spread=0.35):
    """A clustered corpus (fp32 [n, d], not normalised: the cosine writer does that) and unit-length queries near the
    same centres."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((centers, d))
    rows = cent[rng.integers(0, centers, n)] + spread * rng.standard_normal((n, d))
    q = cent[rng.integers(0, centers, nq)] + spread * rng.standard_normal((nq, d))
    return rows.astype(np.float32), S.normalize_rows(q.astype(np.float32))


def duplicated(n=400, d=IX_D, copies=200, seed=IX_SEED + 1):
    """A corpus whose first ``copies`` rows are one vector (more than any R tie for the best place) -> (rows, that query)."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[:copies] = rows[0]
    return rows, S.normalize_rows(rows[:1].copy())
