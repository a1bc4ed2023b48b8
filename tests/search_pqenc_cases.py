"""The cases of the product-quantisation assign tests (HZ_K_SEARCH_PQASSIGN, ``pq_assign_f32``, the ``"f32"`` / ``"gpu"``
backends), shared by the CPU and the GPU files. Inputs come from ``search_bits_cases.mix``, a closed-form integer recipe.
Every case is made once at ``NMAX`` rows; a smaller N is its first rows (the contract: a row's bits do not depend on N),
and ``ref`` computes ``pq_assign_f32`` once per case.

  * ``integer``: rows and centroids are integers in [-4, 4]: every distance is an integer below 2^13, exact in fp32 and
    fp64. Centroids ``DUP`` .. 255 repeat centroids 0 .. 255 - ``DUP``, so every minimum ties at least once and the answer
    is the lower index: no code reaches ``DUP``.
  * ``inexact``: rows of unit norm rounded to bf16, the codebook ``pq_train(iters=2)`` of them.
  * ``neartie``: a sub-vector is one bf16 value v repeated dsub times; centroids 2i and 2i + 1 are v_i + e and
    v_i + reversed(e) for a full-mantissa e of about 2^-7: the two distances sum the SAME dsub squares in opposite
    orders, so they differ by rounding alone (0, 1 or 2 ulps) and which one is smaller is decided by the order of the
    additions and by whether a product is rounded before it is added. The other centroids are far away. The maker
    asserts that the contract's arithmetic and an fmaf chain disagree somewhere (for dsub >= 2: a one-term sum has no
    order, and fma(t, t, +0) rounds exactly as t * t).

No square underflows: |t| is 0 or at least 2^-12 everywhere."""
import functools

import numpy as np

from hipzap import search as S

from search_bits_cases import mix
from search_filter_cases import T, gamma  # noqa: F401  (re-exported)

# (D, M): dsub 8, 16, 8, 64 (the maximum), 1 (the minimum), 3 (odd: sub-vectors are not 16-B aligned), 64 at the D limit
SHAPES = [(768, 96), (768, 48), (128, 16), (1024, 16), (16, 16), (48, 16), (2048, 32)]
NS = (1, T + 1, 3 * T + 5)
NMAX = NS[-1]
KINDS = ("integer", "inexact", "neartie")
DUP = 200
NEAR_VALUES = np.array([0.5, -0.75, 1.25, -1.5, 0.15625, -0.3125, 2.5, -0.09375], np.float32)  # bf16 numbers


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grid(n, d, salt):
    return mix(np.arange(n)[:, None], np.arange(d)[None, :], salt)


def _unit(x):
    """uint64 hashes -> float64 in [0, 1) with 24 random bits."""
    return ((x >> np.uint64(11)) & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)


def fma_chain(rows32, cb):
    """What an FMA-contracted kernel would compute: acc = fma(t, t, acc), emulated in fp64 (t * t is exact there) and
    rounded to fp32 after each step -> (codes [N, M], dist fp32 [N, M]) under the contract's strict-< walk."""
    m, _, dsub = cb.shape
    x = np.asarray(rows32, np.float32).reshape(-1, m, dsub)
    codes = np.empty(x.shape[:2], np.uint8)
    dist = np.empty(x.shape[:2], np.float32)
    for j in range(m):
        acc = np.zeros((x.shape[0], 256), np.float32)
        for i in range(dsub):
            t = (x[:, j, i, None] - cb[j, None, :, i]).astype(np.float64)  # the subtraction is still an fp32 operation
            acc = (t * t + acc.astype(np.float64)).astype(np.float32)
        best = np.argmin(acc, axis=1)
        codes[:, j], dist[:, j] = best, acc[np.arange(x.shape[0]), best]
    return codes, dist


@functools.lru_cache(maxsize=None)
def _make(kind, D, M):
    dsub = D // M
    base = 104729 * D + 1299709 * M
    if kind == "integer":
        rows = (_grid(NMAX, D, base) % np.uint64(9)).astype(np.float32) - np.float32(4)
        cb = (_grid(M * 256, dsub, base + 1) % np.uint64(9)).astype(np.float32).reshape(M, 256, dsub) - np.float32(4)
        cb[:, DUP:] = cb[:, :256 - DUP]
    elif kind == "inexact":
        g = _unit(_grid(NMAX, D, base + 2)) + _unit(_grid(NMAX, D, base + 3)) + _unit(_grid(NMAX, D, base + 4)) - 1.5
        rows = S.bf16_to_f32(S.to_bf16((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)))
        cb = S.pq_train(rows, M, seed=5, iters=2)
    else:
        pick = (_grid(NMAX, M, base + 5) % np.uint64(NEAR_VALUES.size)).astype(np.int64)
        rows = np.repeat(NEAR_VALUES[pick], dsub, axis=1)
        h = _grid(M * 256, dsub, base + 6).reshape(M, 256, dsub)
        far = (10.0 + 4.0 * _unit(h)) * np.where(h & np.uint64(1), 1.0, -1.0)
        cb = far.astype(np.float32)
        e = ((2.0 ** -8 + (2.0 ** -6 - 2.0 ** -8) * _unit(h >> np.uint64(3))) * np.where(h & np.uint64(2), 1.0, -1.0))
        for i, v in enumerate(NEAR_VALUES):
            cb[:, 2 * i] = (np.float64(v) + e[:, i]).astype(np.float32)
            cb[:, 2 * i + 1] = cb[:, 2 * i, ::-1]
    rows = np.ascontiguousarray(rows, np.float32)
    cb = np.ascontiguousarray(cb, np.float32)
    assert np.array_equal(S.bf16_to_f32(S.to_bf16(rows)), rows)
    rows.setflags(write=False)
    cb.setflags(write=False)
    return rows, cb


def make(kind, N, D, M):
    """-> (rows fp32 [N, D], every value a bf16 number; codebook fp32 [M, 256, D / M]). Read-only: shared."""
    rows, cb = _make(kind, D, M)
    return rows[:N], cb


@functools.lru_cache(maxsize=None)
def _ref(kind, D, M):
    rows, cb = _make(kind, D, M)
    codes, dist = S.pq_assign_f32(rows, cb)
    if kind == "neartie" and D // M >= 2:  # the case can catch what it is for
        fc, fd = fma_chain(rows, cb)
        assert (u32(fd) != u32(dist)).any(), "neartie: an fmaf chain gives the contract's distance bits everywhere"
        assert (codes < 2 * NEAR_VALUES.size).all()
    codes.setflags(write=False)
    dist.setflags(write=False)
    return codes, dist


def ref(kind, N, D, M):
    """``pq_assign_f32`` of ``make(kind, N, D, M)`` -> (codes uint8 [N, M], dist fp32 [N, M]); computed once per case."""
    codes, dist = _ref(kind, D, M)
    return codes[:N], dist[:N]


def d64(rows32, cb, codes):
    """The exact squared distance, in fp64 as sum (x - c)^2, of every (row, sub-space) to the centroid ``codes`` names."""
    m, _, dsub = cb.shape
    x = np.asarray(rows32, np.float64).reshape(-1, m, dsub)
    c = cb.astype(np.float64)[np.arange(m)[None, :], np.asarray(codes, np.int64)]
    return ((x - c) ** 2).sum(axis=2)


# index-level scenario (tests/test_search_pqenc_index_gpu.py)
IX_D, IX_M, IX_N, IX_ADD = 128, 16, 2 * T - 40, T + 9


def index_vectors():
    """(A fp32 [IX_N, D], B fp32 [IX_ADD, D]): isotropic unit-norm rows rounded to bf16. A seeded generator, not ``mix``
    (whose rows are strongly correlated: near-duplicates would crowd a row out of its own candidates); nothing recorded
    depends on the values."""
    g = np.random.default_rng(7).standard_normal((IX_N + IX_ADD, IX_D))
    rows = S.bf16_to_f32(S.to_bf16((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)))
    return rows[:IX_N].copy(), rows[IX_N:].copy()
