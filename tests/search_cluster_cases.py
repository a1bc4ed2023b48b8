"""The cases and fp64 oracles of the clustering tests (HZ_K_SEARCH_ASSIGN / HZ_K_SEARCH_CMEAN, ``Index.cluster``),
shared by tests/test_search_cluster_cpu.py and the two GPU files.

Assign bound: every product of two bf16 values is exact in fp32 and a score is D fp32 additions inside and between
MFMAs whose internal rounding is not documented as round-to-nearest, so ``beta(D) * sum_i |c_i r_i|`` with ``beta(D) =
D * 2^-23 / (1 - D * 2^-23)`` (tests/search_neighbors_cases.py) holds for any order and for truncating
adds.

Cmean bound (``cmean_bound``): the kernel adds the m widened bf16 values of a column with round-to-nearest fp32 adds in
some fixed order, so |sum32 - sum| <= gamma(m) * sum|x| with gamma(m) = m u / (1 - m u), u = 2^-24 (Higham, Accuracy
and Stability, eq. 4.4; any order). (float)count is exact (count < 2^24) and the division rounds once: eps_d =
gamma(m) * sum|x_d| / count + u * |mean_d|. With ``cosine`` the kernel divides by n^ = fl(sqrt(fl(sum_d mean^_d^2))) =
||mean^|| (1 + theta), |theta| <= gamma(D + 4) (D squares and D - 1 adds under the root, which halves the relative
error, plus the root's own rounding), and | ||mean^|| - ||mean|| | <= ||eps||. To first order
|v^_d - v_d| <= eps_d / ||mean|| + |v_d| * (||eps|| / ||mean|| + theta) + u * |v_d|; every relative error here is below
2^-12, so the dropped second-order terms are below 2^-12 of the bound and the bound is multiplied by (1 + 2^-10)."""
import numpy as np

from hipzap import search as S

T = 256   # HZ_SEARCH_TILE
CB = 64   # HZ_SEARCH_ASSIGN_CB
U = 2.0 ** -24


def beta(D):
    return D * 2.0 ** -23 / (1 - D * 2.0 ** -23)


def gamma(m):
    return m * U / (1 - m * U)


def live_pattern(name, N):
    """bool [N]: which rows have their bit set."""
    live = np.ones(N, bool)
    if name == "all":
        pass
    elif name == "one_dead":  # a dead row in a mixed group of 16
        live[N // 2] = False
    elif name == "dead_group":  # a whole group of 16 rows, and half of the next one
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


# (name, N, D, C, live pattern, seed): every N of {1, 255, 256, 257, 600}, D of {32, 96, 2048} and C of {1, 63, 64, 65,
# 200} appears; the row states: a dead row in a mixed group, a dead group, a dead tile, the last partial tile
ASSIGN_CASES = [
    ("n1_c1", 1, 32, 1, "all", 0),
    ("n255_c63", 255, 96, 63, "one_dead", 1),
    ("n256_c64_d2048", 256, 2048, 64, "dead_group", 2),
    ("n257_c65", 257, 96, 65, "all", 3),
    ("n600_c200", 600, 96, 200, "dead_tile", 4),
    ("n600_c200_d2048", 600, 2048, 200, "dead_group", 5),
    ("n600_c1_d32", 600, 32, 1, "alternating", 6),
    ("n257_c200_d32", 257, 32, 200, "one_dead", 7),
]
ASSIGN_NAMES = [c[0] for c in ASSIGN_CASES]


def make_assign(N, D, C, seed):
    """Planted data: C random centroids and N rows, each a centroid plus half as much noise -> (row bits [N, D],
    centroid bits [C, D]). The nearest centroid of almost every row is clear of the second by far more than the
    bound (asserted, not assumed, by the tests)."""
    rng = np.random.default_rng(4100 + seed)
    cent = rng.standard_normal((C, D)).astype(np.float32)
    lab = rng.integers(0, C, N)
    rows = cent[lab] + np.float32(0.5) * rng.standard_normal((N, D)).astype(np.float32)
    return S.to_bf16(rows), S.to_bf16(cent)


def build_assign(name):
    """-> (row bits, centroid bits, live bool [N])."""
    for n, N, D, C, pattern, seed in ASSIGN_CASES:
        if n == name:
            rb, cb = make_assign(N, D, C, seed)
            return rb, cb, live_pattern(pattern, N)
    raise KeyError(name)


def scores64(rows_bits, cent_bits):
    """(fp64 scores [N, C], bounds [N, C])."""
    r, c = S.bf16_to_f32(rows_bits).astype(np.float64), S.bf16_to_f32(cent_bits).astype(np.float64)
    return r @ c.T, beta(r.shape[1]) * (np.abs(r) @ np.abs(c).T)


def assign_ref(rows_bits, cent_bits, live):
    """The oracle -> (best index int32 [N], -1 for a dead row; its fp64 score, -inf for a dead row; the second-best
    score, -inf with one centroid). The lowest index among equal scores."""
    s, _ = scores64(rows_bits, cent_bits)
    best = np.argmax(s, axis=1).astype(np.int32)
    top = s[np.arange(s.shape[0]), best]
    rest = s.copy()
    rest[np.arange(s.shape[0]), best] = -np.inf
    second = rest.max(axis=1)
    live = np.asarray(live, bool)
    return np.where(live, best, -1).astype(np.int32), np.where(live, top, -np.inf), second


_ORACLE = {}


def assign_oracle(name):
    if name not in _ORACLE:
        rb, cb, live = build_assign(name)
        _ORACLE[name] = (*scores64(rb, cb), *assign_ref(rb, cb, live))
    return _ORACLE[name]


def unclear(s, b, best, top, second, live):
    """bool [N]: the live rows whose oracle margin (best - second) is within twice the bound."""
    bb = b[np.arange(s.shape[0]), np.maximum(best, 0)]
    with np.errstate(invalid="ignore"):  # a dead row of a one-centroid case: -inf - -inf
        return np.asarray(live, bool) & ~(top - second > 2 * bb)


def check_assign(out_list, out_score, s, b, best, top, second, live):
    """The issue's criteria -> (rows inside the margin, worst |err| / bound)."""
    live = np.asarray(live, bool)
    n = s.shape[0]
    assert (out_list[~live] == -1).all() and (out_score[~live] == -np.inf).all()
    rows = np.flatnonzero(live)
    got = out_list[rows]
    assert ((got >= 0) & (got < s.shape[1])).all(), got
    sg, bg = s[rows, got], b[rows, got]
    assert (sg >= s[rows].max(axis=1) - 2 * bg).all()  # a centroid within twice the bound of the fp64 maximum
    soft = unclear(s, b, best, top, second, live)
    clear = live & ~soft
    assert np.array_equal(out_list[clear], best[clear])
    err = np.abs(out_score[rows].astype(np.float64) - sg)
    assert (err <= bg).all(), (err / np.maximum(bg, 1e-300)).max()
    assert soft.sum() <= 0.01 * n, (int(soft.sum()), n)  # a condition on the input, not on the kernel
    return int(soft.sum()), float((err / np.maximum(bg, 1e-300)).max()) if rows.size else 0.0


# ---------------------------------------------------------------------------------------- cmean
CMEAN_SIZES = (0, 1, 2, 257, 1000)
CMEAN_N = 1300


def make_cmean(D, seed=0, bad_ids=True):
    """-> (row bits [CMEAN_N, D], order int32 [M], seg_off int32 [C + 1]): segments of CMEAN_SIZES members drawn with
    repeats; with ``bad_ids`` two members of the 257-segment name rows outside [0, N)."""
    rng = np.random.default_rng(4200 + seed)
    rows = S.to_bf16((rng.standard_normal((CMEAN_N, D)) + 0.25).astype(np.float32))
    order = rng.integers(0, CMEAN_N, sum(CMEAN_SIZES)).astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(CMEAN_SIZES)]).astype(np.int32)
    if bad_ids:
        order[seg_off[3] + 5] = -1
        order[seg_off[3] + 200] = CMEAN_N
    return rows, order, seg_off


def cmean_ref(rows_bits, order, seg_off, cosine):
    """The update-step oracle in fp64 -> (values [C, D], NaN rows for a segment with no member inside [0, N);
    sum|x| [C, D]; counted members [C])."""
    r = S.bf16_to_f32(rows_bits).astype(np.float64)
    C, D = len(seg_off) - 1, r.shape[1]
    out, sabs, cnt = np.full((C, D), np.nan), np.zeros((C, D)), np.zeros(C, np.int64)
    for c in range(C):
        ids = order[seg_off[c]:seg_off[c + 1]]
        ids = ids[(ids >= 0) & (ids < r.shape[0])]
        cnt[c] = ids.size
        if ids.size:
            out[c], sabs[c] = r[ids].sum(axis=0) / ids.size, np.abs(r[ids]).sum(axis=0)
            if cosine:
                out[c] = out[c] / max(np.sqrt((out[c] * out[c]).sum()), 1e-12)
    return out, sabs, cnt


def cmean_bound(rows_bits, order, seg_off, cosine):
    """|kernel cent32 - cmean_ref| is at most this, [C, D] (the derivation: this module's docstring)."""
    plain, sabs, cnt = cmean_ref(rows_bits, order, seg_off, False)
    C, D = plain.shape
    out = np.zeros((C, D))
    for c in range(C):
        if not cnt[c]:
            continue
        eps = gamma(int(cnt[c])) * sabs[c] / cnt[c] + U * np.abs(plain[c])
        if not cosine:
            out[c] = eps
            continue
        norm = np.sqrt((plain[c] ** 2).sum())
        v = plain[c] / norm
        out[c] = (eps / norm + np.abs(v) * (np.sqrt((eps ** 2).sum()) / norm + gamma(D + 4)) + U * np.abs(v)) * (1 + 2.0 ** -10)
    return out


# ------------------------------------------------------------------------ the index-level scenarios
def planted(seed=41):
    """D = 64, 8 centres = 8 rows of a random orthogonal matrix, 600 rows = centre + 0.02 N(0, 1) per coordinate
    -> (rows fp32 [600, 64], labels [600], init fp32 [8, 64]: the first member of each cluster)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((64, 64)))
    lab = rng.integers(0, 8, 600)
    lab[:8] = np.arange(8)  # every cluster has a member
    rows = (q[:8][lab] + 0.02 * rng.standard_normal((600, 64))).astype(np.float32)
    init = np.stack([rows[np.flatnonzero(lab == c)[0]] for c in range(8)])
    return rows, lab.astype(np.int32), init


def random_rows(N=1000, D=96, seed=43):
    return np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)
