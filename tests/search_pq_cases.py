"""The cases of the product-quantisation tests (HZ_K_SEARCH_PQLUT / HZ_K_SEARCH_PQSCAN, pq8 indexes), shared by the
CPU and the GPU files. Inputs come from ``search_bits_cases.mix``, a closed-form integer recipe: no RNG library, so
nothing drifts with a numpy version.

  * ``lossless``: the codebook's entries are multiples of 1/8 in [-15/8, 15/8] (bf16-exact), every row IS
    ``pq_decode`` of its codes, and the queries are integers in [-8, 8]: every product is a multiple of 1/8 below 16 and
    every sum over D <= 2048 columns is exact in fp32. ``pq_decode(pq_encode(x)) == x``, and PQ search equals exact
    search over the rows, ties by id.
  * ``integer``: codebook entries in [-3, 3], queries in [-4, 4], codes drawn from 8 values per sub-space: every table
    entry and every score is a small integer, exact in fp32, and many rows tie.
  * ``inexact``: codebook and queries are fp32 bit patterns with full 23-bit mantissas over four binades and mixed
    signs, so every fp32 partial sum is inexact and a changed summation order changes bits.

Bounds (csrc/hipzap.h): a table entry is one fmaf chain over dsub products, |lut32 - lut| <= gamma(dsub) sum_j |q_j c_j|;
a score adds M of them, |score - q.x^| <= gamma(dsub + M) sum_i |q_i| |x^_i|, gamma(n) = n u / (1 - n u), u = 2^-24."""
import numpy as np

from hipzap import search as S

from search_bits_cases import mix
from search_filter_cases import T, gamma, subset_ambiguous  # noqa: F401  (re-exported)

SHAPES = [(128, 16), (768, 96), (768, 48), (2048, 32), (64, 16)]  # (D, M) of the table tests
KINDS = ("lossless", "integer", "inexact")
# index-level scenario (tests/test_search_pq_index_gpu.py): D, M, rows written, rows added, queries, k
IX_D, IX_M, IX_N, IX_ADD, IX_Q, IX_K = 128, 16, 2 * T - 40, T, 3, 10
IX_SALT = 0  # the smallest salt for which no query's top-k is ambiguous under the bound (asserted by the CPU test)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grid(n, d, salt):
    return mix(np.arange(n)[:, None], np.arange(d)[None, :], salt)


def _full_mantissa(x):
    """uint64 hashes -> fp32 with a mixed sign, one of four binades (2^-2 .. 2^1) and all 23 mantissa bits."""
    return (((x & np.uint64(1)) << np.uint64(31)) | ((((x >> np.uint64(1)) % np.uint64(4)) + np.uint64(125)) << np.uint64(23)) |
            ((x >> np.uint64(5)) & np.uint64(0x7FFFFF))).astype(np.uint32).view(np.float32)


def make(kind, N, D, M, Q, salt=0):
    """-> (codes uint8 [N, M], codebook fp32 [M, 256, D / M], queries fp32 [Q, D])."""
    dsub = D // M
    base = 7919 * D + 131 * M + 4096 * salt
    x = _grid(M * 256, dsub, base).reshape(M, 256, dsub)
    y = _grid(Q, D, base + 1)
    z = _grid(N, M, base + 2)
    if kind == "lossless":
        cb = ((x % np.uint64(31)).astype(np.float32) - np.float32(15)) / np.float32(8)
        q = (y % np.uint64(17)).astype(np.float32) - np.float32(8)
        codes = (z % np.uint64(256)).astype(np.uint8)
    elif kind == "integer":
        cb = (x % np.uint64(7)).astype(np.float32) - np.float32(3)
        q = (y % np.uint64(9)).astype(np.float32) - np.float32(4)
        codes = ((z % np.uint64(8)) * np.uint64(37) % np.uint64(256)).astype(np.uint8)
    else:
        cb, q = _full_mantissa(x), _full_mantissa(y)
        codes = (z % np.uint64(256)).astype(np.uint8)
    return codes, np.ascontiguousarray(cb, np.float32), np.ascontiguousarray(q, np.float32)


def lut_oracle(q, cb):
    """fp64 table [Q, M, 256] and the bound of the fmaf chain [Q, M, 256]."""
    m, _, dsub = cb.shape
    q64 = np.asarray(q, np.float64).reshape(q.shape[0], m, dsub)
    c64 = cb.astype(np.float64)
    return np.einsum("qmj,mcj->qmc", q64, c64), gamma(dsub) * np.einsum("qmj,mcj->qmc", np.abs(q64), np.abs(c64))


def score_oracle(codes, cb, q):
    """fp64 scores [Q, N] against the reconstructed rows and the contract's bound [Q, N]."""
    m, _, dsub = cb.shape
    x = S.pq_decode(codes, cb).astype(np.float64)
    q64 = np.asarray(q, np.float64)
    return q64 @ x.T, gamma(dsub + m) * (np.abs(q64) @ np.abs(x).T)


def keys_of(sc, ids):
    """(score bits with -0.0 as +0.0, id) pairs as one comparable int64 array [Q, k, 2]."""
    s = np.ascontiguousarray(sc, np.float32) + np.float32(0.0)
    return np.stack([u32(s).astype(np.int64), np.asarray(ids, np.int64)], axis=-1)


def scan_ref(lut32, codes, k, allow=None):
    """The keys HZ_K_SEARCH_PQSCAN + merge must return for the fp32 table ``lut32`` [Q, M, 256]: ``pq_scores_from_lut``
    bit for bit, then the order rule (higher score, then the lower id) over the allowed rows -> int64 [Q, k, 2]."""
    s = S.pq_scores_from_lut(lut32, codes) + np.float32(0.0)
    Q, n = s.shape
    sc = np.full((Q, k), -np.inf, np.float32)
    ids = np.full((Q, k), -1, np.int32)
    for i in range(Q):
        rows = np.arange(n) if allow is None else np.flatnonzero(allow if np.ndim(allow) == 1 else allow[i])
        order = rows[np.argsort(-s[i, rows].astype(np.float64), kind="stable")[:k]]
        sc[i, :order.size], ids[i, :order.size] = s[i, order], order
    return keys_of(sc, ids)


def index_data(salt=IX_SALT):
    """The index scenario under the inner-product metric: (A fp32 [IX_N, D], B fp32 [IX_ADD, D], codebook, queries).
    The vectors are reconstructions of ``inexact`` codes rounded to bf16, so what ``write_index`` encodes is what a bf16
    index of the same vectors stores."""
    codes, cb, q = make("inexact", IX_N + IX_ADD, IX_D, IX_M, IX_Q, salt)
    v = S.bf16_to_f32(S.to_bf16(S.pq_decode(codes, cb)))
    return v[:IX_N].copy(), v[IX_N:].copy(), cb, q


def index_tags(n, first=0):
    return ((np.arange(first, first + n) * 7) % 3).astype(np.uint32)
