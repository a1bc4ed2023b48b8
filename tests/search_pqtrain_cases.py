"""Inputs of the product-quantisation training tests (HZ_K_SEARCH_PQUPDATE, ``pq_means_seq``, ``pq_train(means=)``):
rows whose fp64 sums depend on the order of the additions, the three code patterns and a codebook of sentinels."""
import numpy as np

PATTERNS = ("uniform", "all255", "low16")


def wide_rows(n, d, m, seed=0, span=60):
    """fp32 [n, d] of bf16 numbers (8-bit significands) with random signs: half of them +-2^span exactly, the others with
    exponents spread over 2^-span .. 2^span. The large ones cancel in many clusters, and what is left is the small ones
    that were added while the running sum was small: an fp64 sum in another order differs in its leading bits, so even
    the fp32 means tell summation orders apart. Sub-space 1 holds -0.0 only."""
    rng = np.random.default_rng(seed)
    big = rng.random((n, d)) < 0.5
    x = np.ldexp(np.where(big, 128, rng.integers(128, 256, (n, d))).astype(np.float64),
                 np.where(big, span, rng.integers(-span, span + 1, (n, d))) - 7)
    x = (x * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32)
    dsub = d // m
    x[:, dsub:2 * dsub] = -0.0
    return x


def make_codes(pattern, n, m, seed=1):
    """uint8 [n, m]: uniform over 0..255; every row on centroid 255 (one thread row of one workgroup adds everything,
    the list fills tile after tile); or uniform over 0..15 (one workgroup owns every row, the others copy)."""
    rng = np.random.default_rng(seed)
    if pattern == "all255":
        return np.full((n, m), 255, np.uint8)
    return rng.integers(0, 256 if pattern == "uniform" else 16, (n, m)).astype(np.uint8)


def sentinels(m, dsub):
    """fp32 [m, 256, dsub], every word distinct: a centroid left alone, or copied from the wrong place, shows."""
    return (np.arange(m * 256 * dsub, dtype=np.float32) + 0.5).reshape(m, 256, dsub)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
