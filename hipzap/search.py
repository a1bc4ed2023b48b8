"""Vector search over the embeddings this runtime produces: ``.hzidx`` index files, the GPU
:class:`Index` (csrc/index.cpp + csrc/search.hip) and the fp64 oracle :func:`search_ref`.

torch-free, like :mod:`hipzap.lite`: numpy and ctypes only.

File format ``.hzidx`` (version 1): ``HzIndexHeader`` (csrc/hipzap.h: magic, version, the JSON header's
length, the row block's offset, count, dim, metric), the JSON header ``{"dim", "count", "dtype": "bf16",
"metric": "cosine" | "ip", "model", "embed": {"pooling", "normalize", "dim"} | null, "labels"?}``, zero
padding, then the bf16 rows ``[count][dim]`` at a 4096-aligned offset. Version 2 (written when an index has
tags or deleted rows) adds the JSON keys ``capacity``, ``tags_off`` and ``live_off``: two 4096-aligned blocks
after the rows, ``count`` uint32 tags and the live bitmap (bit ``r & 31`` of word ``r >> 5``). A version-1
file opens as all live with zero tags. Version 3 is an fp8 index (``dtype`` ``"fp8_e4m3"``): the rows are
``[count][dim]`` OCP e4m3fn bytes (``dim % 16 == 0``) and the JSON key ``scales_off`` names a 4096-aligned
block of ``count`` little-endian fp32 scales after them; row r stands for ``scales[r] * decode(codes[r])``
(:func:`prepare_rows_fp8`). ``capacity``, ``tags_off`` and ``live_off`` are present exactly when version 2
would have them, their blocks after the scales. Version 4 is version 3 plus the JSON keys ``"rescore": "bf16"``
and ``rescore_off``: a 4096-aligned block of ``[count][dim]`` bf16 rows after every version-3 block, the rows a
bf16 index of the same vectors holds (``write_index(dtype="fp8", rescore=True)``). A search of such an index is
two-stage (``search(refine=R)``): the fp8 rows give the best R candidates, which are re-scored against the bf16
rows; the best k of them are returned. Version 5 is an IVF index (``write_index(ivf=nlist)``): version 2 whose
rows, tags and live bitmap are stored list by list around ``nlist`` k-means centroids, every list on a tile
boundary (``capacity`` = tiles * 256 stored rows; the padding rows are dead), plus the JSON block ``"ivf"``:
``nlist``, the default ``nprobe``, ``seed``, ``iters`` and the offsets of four 4096-aligned blocks -- ``centroids_off``
(bf16 ``[nlist][dim]``), ``list_off_off`` (int32 ``[nlist + 1]``, offsets into the next table), ``list_tiles_off``
(int32 ``[tiles]``, each list's tile ids) and ``rowid_off`` (int32 ``[capacity]``: the external id of each stored
row, -1 on padding). ``count`` stays the number of vectors; ids, labels and every public call speak external ids
(the row's position in the input of ``write_index``). A search scans the ``nprobe`` lists whose centroids are
nearest to the query (``search(nprobe=...)``; ``"all"`` scans every list and is exact). Version 6 is version 5's
layout with version 3's rows (``dtype`` ``"fp8_e4m3"``): codes uint8 ``[capacity][dim]`` in stored order,
``scales_off`` naming fp32 ``[capacity]`` in stored order (padding rows: code 0, scale 1, dead), the tags, bitmap and
``ivf`` block as in version 5. Version 7 is version 6 plus ``"rescore": "bf16"`` and ``rescore_off``: bf16
``[count][dim]`` in EXTERNAL-ID order (the rows a plain bf16 index of the same vectors holds), the last block of the
file -- stage one's candidates carry external ids, so the second stage reads ``rows[id]``. Both come from
:func:`convert_index`, which trains the lists on the bf16 rows and then quantises. Version 8 is a binary index
(``dtype`` ``"bin_sign"``, ``write_index(dtype="bin")``): version 3's rule set over sign-bit rows -- the row block is
uint32 ``[count][dim / 32]`` (``dim % 128 == 0``, 128..2048), bit ``i & 31`` of word ``i >> 5`` set iff the sign bit
of column ``i`` is clear (the live bitmap's bit convention; ``-0.0`` gives 0), no scales block, ``capacity`` /
``tags_off`` / ``live_off`` present exactly when version 3 would have them. Version 9 is version 8 plus ``"rescore":
"bf16"`` and ``rescore_off`` as in version 4. Stage one of a search scores ``dim - 2 * popcount(query bits xor row
bits)``, an integer, so ties are the normal case and the order rule decides them; ``search(refine=R)`` re-scores the
best R against the bf16 rows exactly as version 4 does (:func:`prepare_rows_bin`). Version 10 is a
product-quantised index (``dtype`` ``"pq8"``, ``write_index(dtype="pq", pq_m=M)``): version 3's rule set over rows of M
code bytes -- the row block is uint8 ``[count][M]``, the JSON block ``"pq": {"m", "ksub": 256, "dsub", "codebook_off"}``
names a 4096-aligned block after the rows holding the fp32 codebook ``[M][256][dim / M]``, no scales block,
``capacity`` / ``tags_off`` / ``live_off`` present exactly when version 3 would have them (``M % 16 == 0``, 16..96,
``dim % M == 0``, ``dim / M`` in 1..64, ``dim <= 2048``). Version 11 is version 10 plus ``"rescore": "bf16"`` and
``rescore_off`` as in version 4. Stage one scores a row by adding M entries of a per-query table of inner products with
the sub-centroids (:func:`pq_lut_ref`, :func:`pq_scores_from_lut`).

A live index (:meth:`Index.add`, ``delete``, ``set_tags``, ``search(filter=...)``, ``save``): ids are row
positions and are never reused; a search returns the top k of the rows that are live and whose tag passes
the query's ``(mask, value)`` filter, ``(tag & mask) == value``.

Order rule (kernels and oracle alike): higher score first; among equal scores the lower row id first;
``-0.0`` counts as ``+0.0``; with fewer than ``k`` rows the slots past ``count`` hold id -1, score -inf.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
import queue
import struct
import threading

import numpy as np

from .ops.search import MAX_K, MAX_Q

MAGIC = b"HZIDX\0\0\1"
VERSION = 1
VERSION2 = 2  # version 1 plus the JSON keys capacity / tags_off / live_off and their two blocks
VERSION3 = 3  # fp8 rows: uint8 codes, the JSON key scales_off and its block; tags / live as in version 2, or absent
VERSION4 = 4  # version 3 plus the JSON keys rescore / rescore_off and the block of bf16 rows they name
VERSION5 = 5  # version 2 stored list by list plus the JSON block ivf and the four blocks it names
VERSION6 = 6  # version 5's layout with version 3's rows: e4m3 codes and fp32 scales for `capacity` stored rows
VERSION7 = 7  # version 6 plus rescore / rescore_off: bf16 rows [count][dim] in external-id order, the last block
VERSION8 = 8  # sign-bit rows: uint32 [count][dim / 32], no scales; tags / live as in version 3, or absent
VERSION9 = 9  # version 8 plus rescore / rescore_off, as version 4 adds them to version 3
VERSION10 = 10  # pq8 rows: uint8 [count][M], the JSON block pq and the codebook block; tags / live as in version 3, or absent
VERSION11 = 11  # version 10 plus rescore / rescore_off, as version 4 adds them to version 3
FP8_VERSIONS, IVF_VERSIONS, RESCORE_VERSIONS = (VERSION3, VERSION4, VERSION6, VERSION7), (VERSION5, VERSION6, VERSION7), \
    (VERSION4, VERSION7, VERSION9, VERSION11)
BIN_VERSIONS = (VERSION8, VERSION9)
PQ_VERSIONS = (VERSION10, VERSION11)
TILE = 256   # HZ_SEARCH_TILE (csrc/hipzap.h): an IVF list starts on a tile boundary
IVF_MAX_LISTS = 65536
IVF_SAMPLE = 256  # k-means trains on at most this many rows per centroid
NEIGHBORS_BLOCK = 1024  # rows per pass of knn_graph: HZ_INDEX_SELF_MAX_Q (csrc/hipzap.h), one native call
IVF_KEYS = ("centroids_off", "list_off_off", "list_tiles_off", "rowid_off")
DTYPES = {"bf16": "bf16", "fp8": "fp8_e4m3", "bin": "bin_sign", "pq": "pq8"}  # write_index(dtype=...) -> the header's "dtype"
FP8 = "fp8_e4m3"
BIN = "bin_sign"
PQ = "pq8"
PQ_KSUB, PQ_MAX_M, PQ_MAX_DSUB = 256, 96, 64  # sub-centroids per sub-space; HZ_SEARCH_PQ_MAX_M, HZ_SEARCH_PQ_MAX_DSUB
PQ_SAMPLE = 65536  # rows pq_train takes at most
METRICS = ("cosine", "ip")
ALIGN = 4096
HEAD = struct.Struct("<8sIIQQII")  # HzIndexHeader: magic, version, json_len, data_off, count, dim, metric


def to_bf16(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; the input must be finite."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _e4m3_table() -> np.ndarray:
    """The value of every e4m3fn code, float32 [256]; 0x7F and 0xFF are NaN."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    mag = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e.astype(np.float64) - 7))
    mag[[0x7F, 0xFF]] = np.nan
    return np.where(c & 0x80, -mag, mag).astype(np.float32)


E4M3 = _e4m3_table()
E4M3_MAX = 448.0
_E4M3_POS = E4M3[:127].astype(np.float64)           # the 127 non-negative finite values, ascending
_E4M3_MID = (_E4M3_POS[:-1] + _E4M3_POS[1:]) / 2     # exact: neighbours differ in their last bit


def e4m3_to_f32(codes) -> np.ndarray:
    """e4m3fn codes (uint8) -> their values, exactly (every finite code is an fp32 value)."""
    return E4M3[np.asarray(codes, np.uint8)]


def to_e4m3(x) -> np.ndarray:
    """Finite values in [-448, 448] -> OCP e4m3fn codes (uint8), round to nearest even, the subnormals
    (step 2^-9) included; the sign of a value that rounds to zero is kept. Never 0x7F / 0xFF."""
    x = np.asarray(x, np.float64)
    a = np.minimum(np.abs(x), E4M3_MAX)
    code = np.searchsorted(_E4M3_MID, a, side="left")  # the midpoints below a: a tie lands on the lower code
    tie = (code < 126) & (_E4M3_MID[np.minimum(code, 125)] == a) & (code & 1 == 1)
    return (code + tie).astype(np.uint8) | (np.signbit(x).astype(np.uint8) << 7)


def _checked_rows(vectors, metric: str, step: int, what: str = "dim") -> np.ndarray:
    """The checks and the cosine normalisation that every stored format shares -> fp32 [N, D]."""
    v = np.asarray(vectors)
    if v.ndim != 2 or v.dtype.kind != "f":
        raise ValueError(f"vectors must be a float array [N, D], got {v.dtype} {list(v.shape)}")
    v = np.ascontiguousarray(v, np.float32)
    n, d = v.shape
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if d < step or d % step or d > 2048:
        raise ValueError(f"{what} must be a multiple of {step} in {step}..2048, got {d}")
    if n < 1 or n >= 2 ** 31:
        raise ValueError(f"count must be in 1..2^31-1, got {n}")
    bad = np.flatnonzero(~np.isfinite(v).all(axis=1))
    if bad.size:
        raise ValueError(f"row {int(bad[0])} has a non-finite value ({bad.size} such rows)")
    if metric == "cosine":
        norm = np.sqrt((v * v).sum(axis=1, dtype=np.float32), dtype=np.float32)
        v = v / np.maximum(norm, np.float32(1e-12))[:, None]
    return v


def prepare_rows(vectors, metric: str) -> np.ndarray:
    """fp32 [N, D] -> the bf16 bit patterns (uint16 [N, D]) an index of ``metric`` stores: the checks, the
    cosine normalisation and the rounding of :func:`write_index` and of ``add`` (one function: the same bits)."""
    rows = to_bf16(_checked_rows(vectors, metric, 8))
    if not np.isfinite(bf16_to_f32(rows)).all():
        raise ValueError("a value overflows bf16")
    return rows


def quantize_rows(v: np.ndarray):
    """fp32 [N, D] as it stands -> (codes uint8 [N, D], scales float32 [N]); see :func:`prepare_rows_fp8`."""
    v = np.ascontiguousarray(v, np.float32)
    amax = np.abs(v).max(axis=1)
    scale = (amax / np.float32(E4M3_MAX)).astype(np.float32)
    scale = np.maximum(scale, np.finfo(np.float32).tiny)
    scale[amax == 0] = np.float32(1.0)
    x = np.clip((v / scale[:, None]).astype(np.float32), np.float32(-E4M3_MAX), np.float32(E4M3_MAX))
    return to_e4m3(x), scale


def prepare_rows_fp8(vectors, metric: str):
    """fp32 [N, D] -> (codes uint8 [N, D], scales float32 [N]), what an fp8 index of ``metric`` stores: the
    checks and the normalisation of :func:`prepare_rows` (D % 16 == 0 here), then per row, in fp32,
    ``scale = max|v| / 448`` (at least the smallest normal; 1 for an all-zero row) and
    ``code = e4m3fn_rne(clamp(v / scale, -448, 448))``. Each row depends on itself only, so ``add(B)`` onto
    an index of A stores the bytes ``write_index(A u B)`` would.
    ``|v - scale * decode(code)| <= scale * max(|v / scale| * 2^-4, 2^-10) * (1 + 2^-10)``."""
    return quantize_rows(_checked_rows(vectors, metric, 16, "dim of an fp8 index"))


def _pack_signs(clear: np.ndarray) -> np.ndarray:
    """bool [N, D] ("sign bit clear") -> uint32 [N, D / 32]: bit i & 31 of word i >> 5."""
    return np.packbits(np.ascontiguousarray(clear, np.uint8), axis=1, bitorder="little").view("<u4").astype(np.uint32)


def binarize(v) -> np.ndarray:
    """fp32 [N, D] (D % 32 == 0) -> sign-bit words uint32 [N, D / 32]: bit ``i & 31`` of word ``i >> 5`` is 1 iff
    the sign bit of column ``i`` is clear. ``-0.0`` gives 0, ``+0.0`` gives 1."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return _pack_signs((u >> np.uint32(31)) == 0)


def binarize_bf16(bits) -> np.ndarray:
    """bf16 bit patterns uint16 [N, D] -> the words :func:`binarize` gives for the fp32 values they were rounded
    from: round-to-nearest-even never changes a sign bit (a value that rounds to zero magnitude keeps its sign)."""
    return _pack_signs((np.ascontiguousarray(bits, np.uint16) >> np.uint16(15)) == 0)


def prepare_rows_bin(vectors, metric: str) -> np.ndarray:
    """fp32 [N, D] -> the sign-bit words (uint32 [N, D / 32]) a binary index of ``metric`` stores: the checks and the
    cosine normalisation of :func:`prepare_rows` (D % 128 == 0 here, 128..2048), then :func:`binarize`. The same
    words as ``binarize_bf16(prepare_rows(vectors, metric))``."""
    return binarize(_checked_rows(vectors, metric, 128, "dim of a binary index"))


_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int32)


def bin_search_ref(words, qbits, dim: int, k: int, allow=None):
    """The oracle of a binary index's first stage: row words uint32 [N, W] against query words uint32 [Q, W] ->
    (scores float64 [Q, k], ids int32 [Q, k]); score = ``dim - 2 * popcount(q xor r)``, an exact integer, under
    the order rule (higher score first, then the lower id). ``allow`` as in :func:`search_ref`."""
    words = np.ascontiguousarray(words, np.uint32)
    qbits = np.ascontiguousarray(qbits, np.uint32)
    n = words.shape[0]
    if allow is not None:
        allow = np.asarray(allow, bool)
    scores = np.full((qbits.shape[0], k), -np.inf)
    ids = np.full((qbits.shape[0], k), -1, np.int32)
    for i, row in enumerate(qbits):
        ham = _POP8[(words ^ row[None, :]).view(np.uint8)].sum(axis=1) if n else np.zeros(0, np.int32)
        s = (dim - 2 * ham).astype(np.int64)
        if allow is None:
            order = np.argsort(-s, kind="stable")[:k]
        else:
            rows = np.flatnonzero(allow if allow.ndim == 1 else allow[i])
            order = rows[np.argsort(-s[rows], kind="stable")[:k]]
        scores[i, :order.size] = s[order]
        ids[i, :order.size] = order
    return scores, ids


def check_pq_shape(dim, m) -> int:
    """The shape rules of product-quantised rows (csrc/hipzap.h) -> dsub = dim / m, or a ValueError that names them."""
    if not _is_int(m) or m % 16 or not 16 <= m <= PQ_MAX_M:
        raise ValueError(f"pq m must be a multiple of 16 in 16..{PQ_MAX_M} (a row is whole 16-byte chunks and one query's "
                         f"table is m KiB of LDS), got {m!r}")
    if not _is_int(dim) or dim < m or dim % m or dim > 2048 or dim // m > PQ_MAX_DSUB:
        raise ValueError(f"dim of a pq index must be a multiple of m = {m} with dim / m in 1..{PQ_MAX_DSUB} and dim <= 2048, "
                         f"got {dim!r}")
    return int(dim) // int(m)


def check_codebook(codebook, dim: int, m: int) -> np.ndarray:
    """``codebook`` as finite fp32 [m, 256, dim / m]."""
    dsub = check_pq_shape(dim, m)
    cb = np.asarray(codebook)
    if cb.shape != (m, PQ_KSUB, dsub) or cb.dtype.kind != "f":
        raise ValueError(f"codebook must be floats [{m}, {PQ_KSUB}, {dsub}], got {cb.dtype} {list(cb.shape)}")
    cb = np.ascontiguousarray(cb, np.float32)
    if not np.isfinite(cb).all():
        raise ValueError("the codebook has a non-finite value")
    return cb


def _pq_nearest(x32: np.ndarray, cent32: np.ndarray):
    """Rows fp32 [n, dsub] against centroids fp32 [256, dsub] -> (the nearest centroid uint8 [n], its squared distance
    float64 [n]): ``|x|^2 + |c|^2 - 2 x.c`` evaluated in fp64, the lower index among equal values."""
    c = cent32.astype(np.float64)
    cn = (c * c).sum(axis=1)
    best = np.empty(x32.shape[0], np.uint8)
    dist = np.empty(x32.shape[0], np.float64)
    for a in range(0, x32.shape[0], 1 << 16):
        x = x32[a:a + (1 << 16)].astype(np.float64)
        d = (x * x).sum(axis=1)[:, None] + cn[None, :] - 2.0 * (x @ c.T)
        i = np.argmin(d, axis=1)  # the first of equal minima
        best[a:a + (1 << 16)], dist[a:a + (1 << 16)] = i, d[np.arange(i.size), i]
    return best, dist


PQ_BACKENDS = ("cpu", "f32", "gpu")


def _check_pq_backend(backend, what: str = "backend"):
    if backend not in PQ_BACKENDS:
        raise ValueError(f"{what} must be one of {PQ_BACKENDS}, got {backend!r}")


def pq_assign_f32(rows32, codebook, *, chunk: int = 4096):
    """HZ_K_SEARCH_PQASSIGN's arithmetic (csrc/hipzap.h) in numpy float32 -> (codes uint8 [N, M], dist float32 [N, M]):
    for row r, sub-space m and centroid c the sum over j = 0 .. dsub-1, ascending, from +0, of t * t with
    t = rows[r][m*dsub + j] - codebook[m][c][j], every subtraction, multiplication and addition one float32 operation
    (numpy fuses nothing); the code is the first of the smallest values walking c upward under a strict ``<``, so a NaN
    never displaces anything and a column whose first value is NaN keeps code 0. The kernel's oracle, bit for bit, and
    the ``"f32"`` backend. ``chunk`` rows at a time: the working set is chunk x 256 floats, whatever N is; the result
    does not depend on it."""
    cb = np.ascontiguousarray(codebook, np.float32)
    x = np.ascontiguousarray(rows32, np.float32)
    if cb.ndim != 3 or cb.shape[1] != PQ_KSUB:
        raise ValueError(f"codebook must be floats [M, {PQ_KSUB}, dsub], got {list(cb.shape)}")
    m, _, dsub = cb.shape
    if x.ndim != 2 or x.shape[1] != m * dsub:
        raise ValueError(f"rows must be [N, {m * dsub}], got {list(x.shape)}")
    if not _is_int(chunk) or chunk < 1:
        raise ValueError(f"chunk must be an integer >= 1, got {chunk!r}")
    n = x.shape[0]
    codes = np.empty((n, m), np.uint8)
    dist = np.empty((n, m), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, n, chunk):
            xa = x[a:a + chunk]
            rows = np.arange(xa.shape[0])
            for j in range(m):
                ct = np.ascontiguousarray(cb[j].T)  # [dsub, 256]
                d = np.zeros((xa.shape[0], PQ_KSUB), np.float32)
                for i in range(dsub):
                    t = xa[:, j * dsub + i, None] - ct[i][None, :]
                    d = d + t * t
                key = d
                if np.isnan(d).any():  # argmin would pick a NaN; the walk never does, unless it starts on one
                    key = np.where(np.isnan(d), np.float32(np.inf), d)
                    key[np.isnan(d[:, 0]), 0] = -np.inf
                best = np.argmin(key, axis=1)  # the first of equal minima
                codes[a:a + chunk, j], dist[a:a + chunk, j] = best, d[rows, best]
    return codes, dist


def _bf16_exact(x32: np.ndarray) -> np.ndarray:
    """fp32 rows -> their bf16 bits, or a ValueError when a value is not a bf16 number (the GPU encoder reads bf16 rows)."""
    if not np.isfinite(x32).all():
        raise ValueError("backend='gpu' needs finite rows")
    bits = to_bf16(x32)
    if not np.array_equal(bf16_to_f32(bits), x32):
        raise ValueError("backend='gpu' needs rows that are exactly representable in bf16 (round them with "
                         "bf16_to_f32(to_bf16(rows)) first, as prepare_rows_pq does)")
    return bits


def _pq_assign(x32: np.ndarray, cb: np.ndarray, backend: str, device: int, chunk_rows: int = 0, bits=None) -> np.ndarray:
    """Codes uint8 [N, M] of ``x32`` by the ``"f32"`` or the ``"gpu"`` backend (``bits``: the rows' bf16 bits, if the
    caller has them already)."""
    if backend == "f32":
        return pq_assign_f32(x32, cb)[0]
    from .ops.search import pq_encode_rows
    return pq_encode_rows(_bf16_exact(x32) if bits is None else bits, cb, device=device, chunk_rows=chunk_rows)[0]


def pq_train(rows32, m: int, *, seed: int = 0, iters: int = 10, sample: int = PQ_SAMPLE, init=None, backend: str = "cpu",
             device: int = 0) -> np.ndarray:
    """Train a product quantiser on ``rows32`` (fp32 [N, D]) -> the codebook, fp32 [m, 256, D / m]. Per sub-space,
    Lloyd's k-means under squared L2 over at most ``sample`` rows: the rows are the first ``sample`` of a seeded
    permutation, in ascending order, the same rows for every sub-space; the first centroids of sub-space j are the
    sub-vectors of 256 of those rows (one more seeded draw, the same rows for every sub-space; with fewer than 256
    rows the remaining centroids are zero). Assignment is :func:`pq_encode`'s (fp64, the lower centroid on ties); a
    centroid becomes its members' mean, accumulated in fp64 in row order and rounded to fp32, and keeps its value
    when it has no member. Deterministic for a given input and seed. ``init`` (fp32 [m, 256, D / m]) replaces the
    first centroids; ``iters=0`` with ``init`` returns it unchanged. ``backend`` changes the assignment step alone:
    ``"f32"`` is :func:`pq_assign_f32`, ``"gpu"`` HZ_K_SEARCH_PQASSIGN on ``device`` over the sample, gathered on the
    host once (one ``hz_pq_encode`` per iteration; the rows must be bf16 numbers) -- the same bits as ``"f32"``, so
    the two give the same codebook bit for bit; the sample, the first centroids and the means are the same code for
    every backend."""
    _check_pq_backend(backend)
    x = np.asarray(rows32)
    if x.ndim != 2 or x.dtype.kind != "f" or x.shape[0] < 1:
        raise ValueError(f"rows must be a float array [N, D] with N >= 1, got {x.dtype} {list(x.shape)}")
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    dsub = check_pq_shape(d, m)
    if not _is_int(iters) or iters < 0 or not _is_int(seed) or seed < 0 or not _is_int(sample) or sample < 1:
        raise ValueError(f"seed and iters must be integers >= 0 and sample >= 1, got {seed!r}, {iters!r}, {sample!r}")
    rng = np.random.default_rng(seed)
    take = np.sort(rng.permutation(n)[:sample])
    first = np.sort(rng.permutation(take.size)[:PQ_KSUB])
    xs = x[take].reshape(take.size, m, dsub)
    if init is None:
        cb = np.zeros((m, PQ_KSUB, dsub), np.float32)
        cb[:, :first.size] = xs[first].transpose(1, 0, 2)
    else:
        cb = check_codebook(init, d, m).copy()
    flat = bits = None
    if backend != "cpu" and iters:
        flat = np.ascontiguousarray(xs.reshape(take.size, d))
        bits = _bf16_exact(flat) if backend == "gpu" else None
    for _ in range(int(iters)):
        codes = None if backend == "cpu" else _pq_assign(flat, cb, backend, device, bits=bits)
        for j in range(m):
            sub = np.ascontiguousarray(xs[:, j])
            a = _pq_nearest(sub, cb[j])[0] if codes is None else codes[:, j]
            order = np.argsort(a, kind="stable")  # ascending rows inside a cluster
            sizes = np.bincount(a, minlength=PQ_KSUB)
            used = np.flatnonzero(sizes)
            starts = np.concatenate([[0], np.cumsum(sizes)])[used]
            sums = np.add.reduceat(sub[order].astype(np.float64), starts, axis=0)
            cb[j, used] = (sums / sizes[used][:, None]).astype(np.float32)
    return cb


def pq_encode(rows32, codebook, *, backend: str = "cpu", device: int = 0, chunk_rows: int = 0) -> np.ndarray:
    """fp32 rows [N, D] -> codes uint8 [N, M]: per sub-space the nearest centroid of ``codebook`` (fp32 [M, 256, D / M])
    by squared L2 evaluated in fp64, the lower index on ties. Works through the rows in chunks, one sub-space at a
    time: 10^6 x 768 needs the input, the codes and a few hundred MB. ``backend="f32"``: the distances in plain
    float32 operations instead (:func:`pq_assign_f32`); ``"gpu"``: those same bits from HZ_K_SEARCH_PQASSIGN on
    ``device`` (``hz_pq_encode``, ``chunk_rows`` rows per device pass, 0 for its default) -- the rows must be bf16
    numbers, anything else is a ValueError. The two agree bit for bit; against the fp64 choice either may pick a
    centroid whose distance is within (1 + g) / (1 - g), g = gamma(dsub + 2), of the optimum."""
    _check_pq_backend(backend)
    cb = np.asarray(codebook, np.float32)
    x = np.ascontiguousarray(rows32, np.float32)
    m, _, dsub = cb.shape
    if x.ndim != 2 or x.shape[1] != m * dsub:
        raise ValueError(f"rows must be [N, {m * dsub}], got {list(x.shape)}")
    if backend != "cpu":
        if x.shape[0] == 0:
            return np.empty((0, m), np.uint8)
        return _pq_assign(x, np.ascontiguousarray(cb), backend, device, chunk_rows)
    codes = np.empty((x.shape[0], m), np.uint8)
    for j in range(m):
        codes[:, j] = _pq_nearest(x[:, j * dsub:(j + 1) * dsub], cb[j])[0]
    return codes


def pq_distortion(rows32, codebook) -> float:
    """The mean squared L2 error of ``pq_decode(pq_encode(rows))`` per row, in fp64."""
    cb = np.asarray(codebook, np.float32)
    x = np.ascontiguousarray(rows32, np.float32)
    m, _, dsub = cb.shape
    return float(sum(_pq_nearest(x[:, j * dsub:(j + 1) * dsub], cb[j])[1].sum() for j in range(m)) / x.shape[0])


def pq_decode(codes, codebook) -> np.ndarray:
    """Codes uint8 [N, M] -> the reconstructed rows, fp32 [N, D]: sub-space m of row r is ``codebook[m][codes[r][m]]``."""
    cb = np.asarray(codebook, np.float32)
    codes = np.asarray(codes, np.uint8)
    m = cb.shape[0]
    return cb[np.arange(m)[None, :], codes].reshape(codes.shape[0], -1)


def pq_lut_ref(q, codebook) -> np.ndarray:
    """The table of the queries ``q`` (fp32 [Q, D]) in fp64 [Q, M, 256]: entry (q, m, c) is the inner product of the
    query's sub-space m with ``codebook[m][c]``."""
    cb = np.asarray(codebook, np.float64)
    q = np.asarray(q, np.float64)
    if q.ndim == 1:
        q = q[None]
    m, _, dsub = cb.shape
    return np.einsum("qmj,mcj->qmc", q.reshape(q.shape[0], m, dsub), cb)


def pq_scores_from_lut(lut32, codes) -> np.ndarray:
    """The scan's arithmetic given a table: fp32 ``lut32`` [Q, M, 256] (or [M, 256]) and codes uint8 [N, M] -> fp32
    scores [Q, N] (or [N]), each the sequential fp32 sum over m = 0 .. M-1 from +0 of ``lut32[q][m][codes[r][m]]`` --
    plain additions, the bits of HZ_K_SEARCH_PQSCAN for that table."""
    lut = np.asarray(lut32, np.float32)
    codes = np.asarray(codes, np.uint8)
    one = lut.ndim == 2
    if one:
        lut = lut[None]
    acc = np.zeros((lut.shape[0], codes.shape[0]), np.float32)
    for j in range(lut.shape[1]):
        acc = acc + lut[:, j, :][:, codes[:, j]]  # float32 + float32: one rounding per addition
    return acc[0] if one else acc


def pq_search_ref(codes, codebook, q, k: int, allow=None):
    """The oracle of a pq8 index's first stage: the exact inner product of each query with each reconstructed row
    (the fp64 table, summed in fp64) -> (scores float64 [Q, k], ids int32 [Q, k]) under the order rule. ``allow`` as in
    :func:`search_ref`."""
    codes = np.asarray(codes, np.uint8)
    lut = pq_lut_ref(q, codebook)
    n, m = codes.shape
    if allow is not None:
        allow = np.asarray(allow, bool)
        if allow.shape not in ((n,), (lut.shape[0], n)):
            raise ValueError(f"allow must be bool [{n}] or [{lut.shape[0]}, {n}], got {list(allow.shape)}")
    scores = np.full((lut.shape[0], k), -np.inf)
    ids = np.full((lut.shape[0], k), -1, np.int32)
    col = np.arange(m)[None, :]
    for i in range(lut.shape[0]):
        s = lut[i][col, codes].sum(axis=1) + 0.0 if n else np.zeros(0)
        if allow is None:
            order = np.argsort(-s, kind="stable")[:k]
        else:
            rows = np.flatnonzero(allow if allow.ndim == 1 else allow[i])
            order = rows[np.argsort(-s[rows], kind="stable")[:k]]
        scores[i, :order.size] = s[order]
        ids[i, :order.size] = order
    return scores, ids


def prepare_rows_pq(vectors, metric: str, m: int, codebook=None, *, seed: int = 0, iters: int = 10,
                    sample: int = PQ_SAMPLE, backend: str = "cpu", device: int = 0):
    """fp32 [N, D] -> (codes uint8 [N, m], codebook fp32 [m, 256, D / m]), what a pq8 index of ``metric`` stores: the
    checks and the cosine normalisation of :func:`prepare_rows`, the rounding to bf16, then :func:`pq_train` over the
    rounded rows (unless ``codebook`` is given) and :func:`pq_encode` against it. Rounding first means that
    ``convert_index`` from a bf16 index and ``write_index`` from the same vectors see the same rows: with the same
    codebook they store the same bytes. ``backend`` / ``device`` go to both (:func:`pq_train`, :func:`pq_encode`)."""
    _check_pq_backend(backend)
    check_pq_shape(np.asarray(vectors).shape[1] if np.asarray(vectors).ndim == 2 else 0, m)
    bits = to_bf16(_checked_rows(vectors, metric, int(m), f"dim of a pq index with m = {m}"))
    rows = bf16_to_f32(bits)
    if not np.isfinite(rows).all():
        raise ValueError("a value overflows bf16")
    cb = pq_train(rows, m, seed=seed, iters=iters, sample=sample, backend=backend, device=device) if codebook is None \
        else check_codebook(codebook, rows.shape[1], m)
    return pq_encode(rows, cb, backend=backend, device=device), cb


def check_tags(tags, n: int) -> np.ndarray:
    """``tags`` as uint32 [n]; integers in 0..2^32-1 only."""
    t = np.asarray(tags)
    if t.ndim != 1 or t.shape[0] != n or t.dtype.kind not in "iu":
        raise ValueError(f"tags must be {n} integers, got {t.dtype} {list(t.shape)}")
    if t.size and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
        raise ValueError("tags must be in 0..2^32-1")
    return np.ascontiguousarray(t.astype(np.uint32))


def pack_live(live) -> np.ndarray:
    """bool [N] -> the live bitmap, uint32 [ceil(N / 32)]: bit r & 31 of word r >> 5."""
    live = np.asarray(live, bool)
    pad = np.zeros(-(-live.size // 32) * 32, np.uint8)
    pad[:live.size] = live
    return np.packbits(pad, bitorder="little").view("<u4").astype(np.uint32)


def unpack_live(words, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def _write_file(path: str, hdr: dict, rows: np.ndarray, tags=None, live=None, capacity=None, scales=None,
                rescore=None, ivf=None, pq=None) -> dict:
    """The file of ``hdr`` and ``rows``: version 1 without ``tags`` / ``live``, else version 2 (zero tags / all
    live where one is missing); with ``scales`` (fp8 rows) version 3, whose tags and bitmap are present under
    the same rule; with ``rescore`` as well (bf16 bit patterns [N, D]) version 4, their block last. With ``ivf``
    (:func:`ivf_layout`'s tables; ``rows``, ``tags`` and ``live`` in stored order, ``hdr["count"]`` the number of
    vectors) version 5, the four tables last; with ``ivf`` and ``scales`` (codes and scales in stored order) version
    6, and with ``rescore`` as well (``[hdr["count"], D]``, in id order) version 7, their block after the tables.
    With ``pq`` (the codebook fp32 [M, 256, dim / M]; ``rows`` uint8 codes [N, M]) version 10, with ``rescore`` as
    well version 11: the codebook's block follows the rows, where version 3 has its scales.
    Atomic: a temporary file, then a rename. Returns the JSON header written."""
    n = rows.shape[0]
    binary = hdr.get("dtype") == BIN  # sign-bit rows: uint32 [N, dim / 32], versions 8 and 9
    if (hdr.get("dtype") == PQ) != (pq is not None):
        raise ValueError("a pq8 index goes with a codebook, and only a pq8 index does")
    if pq is not None:
        pq = check_codebook(pq, hdr["dim"], rows.shape[1] if rows.ndim == 2 else 0)
        if ivf is not None or scales is not None or rows.dtype != np.uint8:
            raise ValueError("a pq8 index holds uint8 rows of m codes, without scales or lists")
    if binary and (ivf is not None or scales is not None or rows.dtype != np.uint32 or rows.shape[1] * 32 != hdr["dim"]):
        raise ValueError("a binary index holds uint32 rows of dim / 32 words, without scales or lists")
    rshape = rows.shape if ivf is None else (hdr["count"], rows.shape[1])
    if binary or pq is not None:
        rshape = (n, hdr["dim"])
    if rescore is not None and ((scales is None and not binary and pq is None) or rescore.shape != rshape or rescore.dtype != np.uint16):
        raise ValueError("rescore rows go with fp8 rows of the same shape")

    def align(x):
        return -(-x // ALIGN) * ALIGN
    if ivf is not None and (tags is None or live is None or n % TILE):
        raise ValueError("an IVF index holds rows, tags and a live bitmap for whole tiles")
    blocks = tags is not None or live is not None
    tables = ()  # the four blocks of an IVF index
    if not blocks and scales is None and not binary and pq is None:
        version, js = VERSION, json.dumps(hdr).encode()
        data_off = align(HEAD.size + len(js))
    else:
        if ivf is not None:
            version = VERSION5 if scales is None else VERSION6 if rescore is None else VERSION7
        elif binary:
            version = VERSION8 if rescore is None else VERSION9
        elif pq is not None:
            version = VERSION10 if rescore is None else VERSION11
            hdr = dict(hdr, pq={"m": int(pq.shape[0]), "ksub": PQ_KSUB, "dsub": int(pq.shape[2]), "codebook_off": 0})
        else:
            version = VERSION2 if scales is None else VERSION3 if rescore is None else VERSION4
        if scales is not None:
            hdr = dict(hdr, scales_off=0)
        if blocks:
            tags = np.zeros(n, np.uint32) if tags is None else tags
            words = pack_live(np.ones(n, bool) if live is None else live)
            hdr = dict(hdr, capacity=int(max(capacity or 0, n)), tags_off=0, live_off=0)
        if rescore is not None:
            hdr = dict(hdr, rescore="bf16", rescore_off=0)
        if ivf is not None:
            tables = (np.ascontiguousarray(ivf["centroids"]).astype("<u2"), np.asarray(ivf["list_off"]).astype("<i4"),
                      np.asarray(ivf["list_tiles"]).astype("<i4"), np.asarray(ivf["rowid"]).astype("<i4"))
            hdr = dict(hdr, ivf=dict({k: int(ivf[k]) for k in ("nlist", "nprobe", "seed", "iters")},
                                     **{k: 0 for k in IVF_KEYS}))
        while True:  # the offsets follow the JSON's own length: a few rounds until they agree
            js = json.dumps(hdr).encode()
            data_off = align(HEAD.size + len(js))
            end = data_off + rows.nbytes
            offs = {}
            if scales is not None:
                offs["scales_off"] = align(end)
                end = offs["scales_off"] + 4 * n
            if pq is not None:
                cb_off = align(end)
                end = cb_off + pq.nbytes
            if blocks:
                offs["tags_off"] = tags_off = align(end)
                offs["live_off"] = live_off = align(tags_off + 4 * n)
                end = live_off + words.nbytes
            if rescore is not None and ivf is None:
                offs["rescore_off"] = align(end)
            ioffs = {}
            for key, block in zip(IVF_KEYS, tables):
                ioffs[key] = align(end)
                end = ioffs[key] + block.nbytes
            if rescore is not None and ivf is not None:  # version 7: the rescore rows are the last block
                offs["rescore_off"] = align(end)
            if all(hdr[k] == v for k, v in offs.items()) and all(hdr["ivf"][k] == v for k, v in ioffs.items()) \
                    and (pq is None or hdr["pq"]["codebook_off"] == cb_off):
                break
            hdr.update(offs)
            if pq is not None:
                hdr["pq"] = dict(hdr["pq"], codebook_off=cb_off)
            if ioffs:
                hdr["ivf"].update(ioffs)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(HEAD.pack(MAGIC, version, len(js), data_off, n if ivf is None else hdr["count"],
                          hdr["dim"] if binary or pq is not None else rows.shape[1], METRICS.index(hdr["metric"])))
        f.write(js)
        f.write(bytes(data_off - HEAD.size - len(js)))
        f.write(rows.astype("<u4").tobytes() if binary else rows.tobytes())
        at = data_off + rows.nbytes
        if scales is not None:
            f.write(bytes(hdr["scales_off"] - at))
            f.write(np.asarray(scales).astype("<f4").tobytes())
            at = hdr["scales_off"] + 4 * n
        if pq is not None:
            f.write(bytes(cb_off - at))
            f.write(pq.astype("<f4").tobytes())
            at = cb_off + pq.nbytes
        if blocks:
            f.write(bytes(tags_off - at))
            f.write(tags.astype("<u4").tobytes())
            f.write(bytes(live_off - tags_off - 4 * n))
            f.write(words.astype("<u4").tobytes())
            at = live_off + words.nbytes
        for key, block in zip(IVF_KEYS, tables):
            f.write(bytes(hdr["ivf"][key] - at))
            f.write(block.tobytes())
            at = hdr["ivf"][key] + block.nbytes
        if rescore is not None:
            f.write(bytes(hdr["rescore_off"] - at))
            f.write(np.ascontiguousarray(rescore).astype("<u2").tobytes())
    os.replace(tmp, path)
    return hdr


def _nearest_centroid(rows32: np.ndarray, cent32: np.ndarray) -> np.ndarray:
    """The centroid of largest inner product per row (the lowest index among equals), int32 [N]; fp32, in blocks."""
    out = np.empty(rows32.shape[0], np.int32)
    step = max(1, (1 << 24) // max(cent32.shape[0], 1))
    for a in range(0, rows32.shape[0], step):
        out[a:a + step] = np.argmax(rows32[a:a + step] @ cent32.T, axis=1)
    return out


def check_init(init, nlist: int, dim: int) -> np.ndarray:
    """``init`` of :func:`ivf_kmeans` / ``cluster``: starting centroids, a finite floating-point [nlist, dim] array
    -> fp32."""
    a = np.asarray(init)
    if a.dtype.kind != "f":
        raise ValueError(f"init must be a floating-point array, got dtype {a.dtype}")
    if a.shape != (nlist, dim):
        raise ValueError(f"init must have the shape [nlist, dim] = [{nlist}, {dim}], got {list(a.shape)}")
    bad = np.argwhere(~np.isfinite(a))
    if bad.size:
        r, c = (int(v) for v in bad[0])
        raise ValueError(f"init must be finite, got {a[r, c]!r} at [{r}, {c}]")
    return np.ascontiguousarray(a, np.float32)


def ivf_kmeans(rows32: np.ndarray, nlist: int, metric: str, seed: int = 0, iters: int = 10, init=None):
    """k-means over the stored rows (bf16 values as fp32 [N, D]) -> (centroid bf16 bits uint16 [nlist, D], the list
    of every row int32 [N]). Trains on at most ``IVF_SAMPLE`` rows per centroid, drawn with ``seed``; the first
    centroids are ``nlist`` distinct sample rows. Assignment is by the largest inner product with the bf16-rounded
    centroids; ``cosine``: spherical k-means (a centroid is its members' mean divided by its norm), ``ip``: plain
    means. A centroid that loses every member keeps its value. Lists may be empty. ``init`` (fp32 [nlist, D]): the
    starting centroids in place of the random draw of rows (the sample is drawn as without it)."""
    rng = np.random.default_rng(seed)
    n = rows32.shape[0]
    m = min(n, IVF_SAMPLE * nlist)
    sample = rows32[np.sort(rng.choice(n, m, replace=False))] if m < n else rows32
    cent = sample[np.sort(rng.choice(m, nlist, replace=False))].astype(np.float32)
    if init is not None:
        cent = check_init(init, nlist, rows32.shape[1]).copy()
    for _ in range(int(iters)):
        a = _nearest_centroid(sample, bf16_to_f32(to_bf16(cent)))
        order = np.argsort(a, kind="stable")
        lists, starts, sizes = np.unique(a[order], return_index=True, return_counts=True)
        sums = np.add.reduceat(sample[order].astype(np.float64), starts, axis=0)
        mean = (sums / sizes[:, None]).astype(np.float32)
        if metric == "cosine":
            mean = mean / np.maximum(np.sqrt((mean * mean).sum(axis=1, dtype=np.float32)), np.float32(1e-12))[:, None]
        cent[lists] = mean
    bits = to_bf16(cent)
    return bits, _nearest_centroid(rows32, bf16_to_f32(bits))


def ivf_layout(assign: np.ndarray, nlist: int) -> dict:
    """The stored order of an IVF index whose row ``i`` belongs to list ``assign[i]``: list after list, each list's
    rows in ascending id and starting on a tile boundary -> ``list_off`` int32 [nlist + 1], ``list_tiles`` int32
    [tiles] (list l's tiles are ``list_tiles[list_off[l]:list_off[l + 1]]``) and ``rowid`` int32 [tiles * TILE]
    (the id of each stored row, -1 on padding)."""
    sizes = np.bincount(assign, minlength=nlist)
    ntiles = -(-sizes // TILE)
    list_off = np.concatenate([[0], np.cumsum(ntiles)]).astype(np.int32)
    rowid = np.full(int(list_off[-1]) * TILE, -1, np.int32)
    order = np.argsort(assign, kind="stable")  # ascending ids inside a list
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    lists = assign[order]
    rowid[list_off[lists].astype(np.int64) * TILE + (np.arange(order.size) - first[lists])] = order
    return {"list_off": list_off, "list_tiles": np.arange(int(list_off[-1]), dtype=np.int32), "rowid": rowid}


def write_index(path: str, vectors, metric: str = "cosine", labels=None, model: str = "", embed=None, tags=None,
                dtype: str = "bf16", rescore: bool = False, ivf=None, nprobe=None, ivf_seed: int = 0,
                ivf_iters: int = 10, ivf_backend: str = "cpu", device: int = 0, pq_m=None, pq_codebook=None,
                pq_seed: int = 0, pq_iters: int = 10, pq_backend: str = "cpu") -> dict:
    """Write ``vectors`` (fp32 [N, D]) as a ``.hzidx`` file and return its JSON header. ``cosine`` rows are
    divided by max(||v||, 1e-12) in fp32 and then rounded to bf16; ``ip`` rows are only rounded. Without
    ``tags`` the file is version 1; with them (uint32 [N]) version 2. ``dtype="fp8"``: e4m3fn rows with one
    scale per row (:func:`prepare_rows_fp8`), a version-3 file; with ``rescore=True`` a version-4 file, which
    also holds the rows of the bf16 index of the same vectors (:func:`prepare_rows`) for the second stage.
    ``ivf=nlist``: an IVF index, a version-5 file -- the rows a plain bf16 index stores (the same bits), grouped
    into ``nlist`` lists by :func:`ivf_kmeans` (``ivf_seed``, ``ivf_iters``) and stored in :func:`ivf_layout`'s order;
    ``nprobe``: the lists a search scans by default, ``min(nlist, 16)`` when None. Ids stay the positions in
    ``vectors``. ``ivf_backend="gpu"``: the lists come from :meth:`Index.cluster` on ``device`` (:func:`cluster_rows`)
    in place of :func:`ivf_kmeans`; the file has the same layout either way. ``dtype="bin"``: sign-bit rows
    (:func:`prepare_rows_bin`), a version-8 file, with ``rescore=True`` version 9. ``dtype="pq"``: rows of ``pq_m``
    code bytes and their codebook (:func:`prepare_rows_pq`: trained with ``pq_seed`` / ``pq_iters`` unless
    ``pq_codebook`` is given), a version-10 file, with ``rescore=True`` version 11; ``pq_backend`` (``"cpu"``,
    ``"f32"``, ``"gpu"`` on ``device``) picks how training and encoding find the nearest sub-centroids
    (:func:`pq_encode`): ``"f32"`` and ``"gpu"`` write the same bytes."""
    _check_ivf_backend(ivf_backend, ivf)
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {tuple(DTYPES)}, got {dtype!r}")
    _check_pq_backend(pq_backend, "pq_backend")
    if dtype != "pq" and (pq_m is not None or pq_codebook is not None or pq_seed != 0 or pq_iters != 10 or pq_backend != "cpu"):
        raise ValueError(f"pq_m, pq_codebook, pq_seed, pq_iters and pq_backend go with dtype='pq', got dtype={dtype!r}")
    if ivf is not None and dtype == "pq":
        raise ValueError(f"ivf={ivf!r} with dtype='pq': IVF lists over pq8 rows are not built")
    if ivf is not None and dtype == "bin":
        raise ValueError(f"ivf={ivf!r} with dtype='bin': IVF lists over binary rows are not built")
    if ivf is not None and (dtype != "bf16" or rescore):
        raise ValueError(f"ivf={ivf!r} goes with dtype='bf16' without rescore rows, got dtype={dtype!r}, rescore={rescore!r}: "
                         f"an fp8 or two-stage IVF index is convert_index(bf16 IVF file, dst, 'fp8', rescore=...)")
    if rescore and dtype not in ("fp8", "bin", "pq"):
        raise ValueError(f"rescore rows go with an fp8 index: a {dtype} index already holds its rows in bf16")
    codebook = None
    if dtype == "pq":
        if pq_m is None:
            raise ValueError("dtype='pq' needs pq_m, the code bytes per row (a multiple of 16 in 16..96 that divides dim)")
        (rows, codebook), scales = prepare_rows_pq(vectors, metric, pq_m, pq_codebook, seed=pq_seed, iters=pq_iters,
                                                   backend=pq_backend, device=device), None
    elif dtype == "bin":
        rows, scales = prepare_rows_bin(vectors, metric), None
    else:
        rows, scales = (prepare_rows(vectors, metric), None) if dtype == "bf16" else prepare_rows_fp8(vectors, metric)
    rrows = prepare_rows(vectors, metric) if rescore else None
    n, d = rows.shape
    if dtype == "bin":
        d *= 32
    if dtype == "pq":
        d = int(np.asarray(vectors).shape[1])
    if labels is not None:
        labels = [str(s) for s in labels]
        if len(labels) != n:
            raise ValueError(f"{len(labels)} labels for {n} rows")
    if tags is not None:
        tags = check_tags(tags, n)
    hdr = {"dim": d, "count": n, "dtype": DTYPES[dtype], "metric": metric, "model": str(model or ""),
           "embed": dict(embed) if embed else None}
    if labels is not None:
        hdr["labels"] = labels
    if ivf is not None:
        nlist, nprobe = _check_ivf_args(n, ivf, nprobe, ivf_seed, ivf_iters)
        cbits, assign = _ivf_lists(rows, nlist, metric, int(ivf_seed), int(ivf_iters), ivf_backend, device, path)
        lay = ivf_layout(assign, nlist)
        real = lay["rowid"] >= 0
        srows = np.zeros((real.size, d), np.uint16)
        srows[real] = rows[lay["rowid"][real]]
        stags = np.zeros(real.size, np.uint32)
        if tags is not None:
            stags[real] = tags[lay["rowid"][real]]
        lay.update(centroids=cbits, nlist=nlist, nprobe=int(nprobe), seed=int(ivf_seed), iters=int(ivf_iters))
        return _write_file(path, hdr, srows, stags, real, ivf=lay)
    return _write_file(path, hdr, rows, tags, scales=scales, rescore=rrows, pq=codebook)


IVF_BACKENDS = ("cpu", "gpu")


def _check_ivf_backend(ivf_backend, ivf):
    if ivf_backend not in IVF_BACKENDS:
        raise ValueError(f"ivf_backend must be one of {IVF_BACKENDS}, got {ivf_backend!r}")
    if ivf is None and ivf_backend != "cpu":
        raise ValueError(f"ivf_backend={ivf_backend!r} goes with ivf=nlist")


def cluster_rows(bits: np.ndarray, nlist: int, metric: str, seed: int = 0, iters: int = 10, device: int = 0,
                 near: str | None = None):
    """:func:`ivf_kmeans` on the GPU: the bf16 rows ``bits`` (uint16 [N, D], D % 32 == 0) are written as a temporary
    plain index (next to ``near``, or in the temporary directory), opened, and clustered with :meth:`Index.cluster`
    -> (centroid bits uint16 [nlist, D], the list of every row int32 [N])."""
    import tempfile
    if bits.shape[1] % 32:
        raise ValueError(f"ivf_backend='gpu' needs dim % 32 == 0 (one MFMA step is 32 columns), got dim = {bits.shape[1]}")
    where = os.path.dirname(os.path.abspath(near)) if near else None
    fd, tmp = tempfile.mkstemp(suffix=".hzidx", prefix=".cluster-", dir=where)
    os.close(fd)
    try:
        _write_file(tmp, {"dim": int(bits.shape[1]), "count": int(bits.shape[0]), "dtype": "bf16", "metric": metric,
                          "model": "", "embed": None}, bits)
        with Index(tmp, device, contexts=1) as ix:
            cbits, assign, _ = ix.cluster(nlist, iters=iters, seed=seed)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return cbits, assign


def _ivf_lists(bits, nlist, metric, seed, iters, backend, device, near):
    if backend == "gpu":
        return cluster_rows(bits, nlist, metric, seed, iters, device, near)
    return ivf_kmeans(bf16_to_f32(bits), nlist, metric, seed, iters)


def _check_ivf_args(n: int, ivf, nprobe, ivf_seed, ivf_iters):
    """The ranges of ``write_index(ivf=, nprobe=, ivf_seed=, ivf_iters=)`` over ``n`` rows -> (nlist, nprobe)."""
    if not _is_int(ivf) or not 1 <= ivf <= min(n, IVF_MAX_LISTS):
        raise ValueError(f"ivf must be an integer in 1..min(count, {IVF_MAX_LISTS}) = 1..{min(n, IVF_MAX_LISTS)}, got {ivf!r}")
    nlist = int(ivf)
    if nprobe is None:
        nprobe = min(nlist, 16)
    if not _is_int(nprobe) or not 1 <= nprobe <= min(nlist, MAX_K):
        raise ValueError(f"nprobe must be an integer in 1..min(ivf, {MAX_K}) = 1..{min(nlist, MAX_K)}, got {nprobe!r}")
    if not _is_int(ivf_seed) or ivf_seed < 0 or not _is_int(ivf_iters) or ivf_iters < 0:
        raise ValueError(f"ivf_seed and ivf_iters must be integers >= 0, got {ivf_seed!r}, {ivf_iters!r}")
    return nlist, int(nprobe)


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def read_header(path: str) -> dict:
    """The JSON header of a ``.hzidx`` file, checked against the fixed head; plus ``data_off``."""
    with open(path, "rb") as f:
        raw = f.read(HEAD.size)
        if len(raw) < HEAD.size or raw[:8] != MAGIC:
            raise ValueError(f"{path} is not a .hzidx file")
        _, version, json_len, data_off, count, dim, metric = HEAD.unpack(raw)
        if version not in (VERSION, VERSION2, VERSION3, VERSION4, VERSION5, VERSION6, VERSION7, VERSION8, VERSION9,
                           VERSION10, VERSION11):
            raise ValueError(f"{path}: unknown .hzidx version {version}")
        hdr = json.loads(f.read(json_len))
        size = os.fstat(f.fileno()).st_size
    if metric >= len(METRICS) or (hdr.get("dim"), hdr.get("count"), hdr.get("metric")) != (dim, count, METRICS[metric]) \
            or hdr.get("dtype") not in DTYPES.values():
        raise ValueError(f"{path}: the JSON header disagrees with the file head")
    fp8 = version in FP8_VERSIONS
    if (hdr["dtype"] == FP8) != fp8:
        raise ValueError(f"{path}: dtype {hdr['dtype']} in a version-{version} file (version 3 means fp8_e4m3 rows, and so do "
                         f"versions 4, 6 and 7)")
    binary = version in BIN_VERSIONS
    if (hdr["dtype"] == BIN) != binary:
        raise ValueError(f"{path}: dtype {hdr['dtype']} in a version-{version} file (versions 8 and 9 mean bin_sign rows, and no "
                         f"other version does)")
    pq = version in PQ_VERSIONS
    if (hdr["dtype"] == PQ) != pq:
        raise ValueError(f"{path}: dtype {hdr['dtype']} in a version-{version} file (versions 10 and 11 mean pq8 rows, and no "
                         f"other version does)")
    if pq:
        blk = hdr.get("pq")
        if not isinstance(blk, dict) or not all(_is_int(blk.get(k)) for k in ("m", "ksub", "dsub", "codebook_off")):
            raise ValueError(f"{path}: a version-{version} file without a pq block of integers m, ksub, dsub, codebook_off")
        if blk["ksub"] != PQ_KSUB:
            raise ValueError(f"{path}: pq ksub must be {PQ_KSUB}, got {blk['ksub']}")
        try:
            dsub = check_pq_shape(dim, blk["m"])
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None
        if blk["dsub"] != dsub:
            raise ValueError(f"{path}: pq dsub {blk['dsub']} is not dim / m = {dsub}")
        if "ivf" in hdr:
            raise ValueError(f"{path}: an ivf block in a version-{version} file: IVF lists over pq8 rows are not built")
    elif "pq" in hdr:
        raise ValueError(f"{path}: a pq block belongs to the files of versions 10 and 11 and to no other (version {version})")
    if version in RESCORE_VERSIONS and (hdr.get("rescore") != "bf16" or "rescore_off" not in hdr):
        raise ValueError(f"{path}: a version-{version} file without rescore / rescore_off")
    if version not in RESCORE_VERSIONS and ("rescore" in hdr or "rescore_off" in hdr):
        raise ValueError(f"{path}: rescore keys in a version-{version} file (they belong to versions "
                         f"{'4, 7, 9 and 11' if pq else '4, 7 and 9' if binary else '4 and 7'})")
    if binary and (dim < 128 or dim % 128 or dim > 2048):
        raise ValueError(f"{path}: dim of a binary index must be a multiple of 128 in 128..2048, got {dim}")
    if fp8 and (dim < 16 or dim % 16 or dim > 2048):
        raise ValueError(f"{path}: dim of an fp8 index must be a multiple of 16 in 16..2048, got {dim}")
    if hdr.get("labels") is not None and len(hdr["labels"]) != count:
        raise ValueError(f"{path}: {len(hdr['labels'])} labels for {count} rows")
    ivf = hdr.get("ivf")
    is_ivf = version in IVF_VERSIONS
    if is_ivf != (ivf is not None):
        raise ValueError(f"{path}: an ivf block belongs to the files of versions 5, 6 and 7 and to no other (version {version})")
    stored = count  # rows in the file's blocks
    if is_ivf:
        stored = hdr.get("capacity")
        if not _is_int(stored) or stored < count or stored % TILE or stored >= 2 ** 31:
            raise ValueError(f"{path}: capacity {stored!r} of an IVF index is not a whole number of tiles holding {count} rows")
        if not isinstance(ivf, dict) or not all(_is_int(ivf.get(k)) for k in ("nlist", "nprobe", "seed", "iters") + IVF_KEYS):
            raise ValueError(f"{path}: the ivf block lacks one of nlist, nprobe, seed, iters, {', '.join(IVF_KEYS)}")
        if not 1 <= ivf["nlist"] <= min(count, IVF_MAX_LISTS) or not 1 <= ivf["nprobe"] <= min(ivf["nlist"], MAX_K):
            raise ValueError(f"{path}: ivf nlist {ivf['nlist']} / nprobe {ivf['nprobe']} out of range for {count} rows")
    end = data_off + stored * dim * (1 if fp8 else 2)
    if binary:
        end = data_off + stored * (dim // 8)
        if data_off % ALIGN or data_off < HEAD.size + json_len or end > size:
            raise ValueError(f"{path}: the row block at {data_off} is unaligned, overlaps the header or lies outside the file")
        if ("tags_off" in hdr) != ("live_off" in hdr):
            raise ValueError(f"{path}: a version-{version} file with only one of tags_off / live_off")
    if pq:
        end = data_off + stored * hdr["pq"]["m"]
        if data_off % ALIGN or data_off < HEAD.size + json_len or end > size:
            raise ValueError(f"{path}: the row block at {data_off} is unaligned, overlaps the header or lies outside the file")
        off, nbytes = hdr["pq"]["codebook_off"], 4 * PQ_KSUB * dim
        if off % ALIGN or off < end or off + nbytes > size:
            raise ValueError(f"{path}: the codebook block at {off} is unaligned, overlaps the rows (which end at {end}) or lies "
                             f"outside the file")
        end = off + nbytes
        if ("tags_off" in hdr) != ("live_off" in hdr):
            raise ValueError(f"{path}: a version-{version} file with only one of tags_off / live_off")
    if fp8:
        off = hdr.get("scales_off")
        if not isinstance(off, int) or off % ALIGN:
            raise ValueError(f"{path}: scales_off {off!r} is not a multiple of {ALIGN}")
        if off < end:
            raise ValueError(f"{path}: the scales block at {off} overlaps the rows, which end at {end}")
        if off + 4 * stored > size:
            raise ValueError(f"{path}: the scales block lies outside the file")
        end = off + 4 * stored
        if ("tags_off" in hdr) != ("live_off" in hdr):
            raise ValueError(f"{path}: a version-{version} file with only one of tags_off / live_off")
    last = end  # the end of the last block before a rescore block
    if version == VERSION2 or is_ivf or ((fp8 or binary or pq) and "tags_off" in hdr):
        for key, nbytes in (("tags_off", 4 * stored), ("live_off", 4 * (-(-stored // 32)))):
            off = hdr.get(key)
            if not isinstance(off, int) or off % ALIGN or off < end or off + nbytes > size:
                raise ValueError(f"{path}: the {key[:4]} block lies outside the file")
            last = max(last, off + nbytes)
        if not isinstance(hdr.get("capacity"), int) or hdr["capacity"] < count:
            raise ValueError(f"{path}: capacity below count")
    if is_ivf:
        sizes = (2 * ivf["nlist"] * dim, 4 * (ivf["nlist"] + 1), 4 * (stored // TILE), 4 * stored)
        for key, nbytes in zip(IVF_KEYS, sizes):
            off = ivf[key]
            if off % ALIGN or off < last or off + nbytes > size:
                raise ValueError(f"{path}: the ivf block {key[:-4]} at {off} is unaligned, overlaps another block or lies "
                                 f"outside the file")
            last = off + nbytes
    if version in RESCORE_VERSIONS:  # after every other block; [count][dim] whatever the stored order
        off = hdr["rescore_off"]
        if not isinstance(off, int) or isinstance(off, bool) or off % ALIGN:
            raise ValueError(f"{path}: rescore_off {off!r} is not a multiple of {ALIGN}")
        if off < last:
            raise ValueError(f"{path}: the rescore block at {off} overlaps another block, which ends at {last}")
        if off + 2 * count * dim > size:
            raise ValueError(f"{path}: the rescore block lies outside the file")
    return dict(hdr, data_off=int(data_off))


def stored_rows(hdr: dict) -> int:
    """Rows in the file's row, tag and live blocks: ``count``, or an IVF index's ``capacity`` (whole tiles, stored
    list by list -- its blocks are in stored order, :func:`read_ivf`'s ``rowid`` gives each stored row's id)."""
    return hdr["capacity"] if "ivf" in hdr else hdr["count"]


def read_tags(path: str) -> np.ndarray:
    """The tag words, uint32 [count] (zeros for a version-1 file)."""
    hdr = read_header(path)
    if "tags_off" not in hdr:
        return np.zeros(hdr["count"], np.uint32)
    return np.fromfile(path, "<u4", stored_rows(hdr), offset=hdr["tags_off"]).astype(np.uint32)


def read_live(path: str) -> np.ndarray:
    """Liveness per row, bool [count] (all live for a version-1 file)."""
    hdr = read_header(path)
    if "live_off" not in hdr:
        return np.ones(hdr["count"], bool)
    n = stored_rows(hdr)
    return unpack_live(np.fromfile(path, "<u4", -(-n // 32), offset=hdr["live_off"]), n)


def file_info(path: str) -> dict:
    """What ``hipzap info`` adds to the header: the format version, capacity, live rows, tags presence."""
    hdr = read_header(path)
    v2 = "tags_off" in hdr
    info = {"version": VERSION2 if v2 else VERSION, "capacity": hdr.get("capacity", hdr["count"]),
            "live": int(read_live(path).sum()), "tags": v2}
    if "ivf" in hdr:
        info.update(version=VERSION5, ivf=ivf_facts(hdr, read_ivf(path)))
    if hdr["dtype"] == FP8:
        info.update(version=VERSION3, dtype=FP8)
    if "rescore_off" in hdr:
        info.update(version=VERSION4, rescore=hdr["rescore"])
    if "ivf" in hdr and hdr["dtype"] == FP8:
        info.update(version=VERSION7 if "rescore_off" in hdr else VERSION6)
    if hdr["dtype"] == BIN:
        info.update(version=VERSION9 if "rescore_off" in hdr else VERSION8, dtype=BIN)
    if hdr["dtype"] == PQ:
        info.update(version=VERSION11 if "rescore_off" in hdr else VERSION10, dtype=PQ,
                    pq={"m": hdr["pq"]["m"], "dsub": hdr["pq"]["dsub"], "codebook_bytes": 4 * PQ_KSUB * hdr["dim"]})
    return info


def read_rows(path: str) -> np.ndarray:
    """The row block: bf16 bit patterns, uint16 [count, dim]; e4m3fn codes, uint8, for an fp8 index; sign-bit
    words, uint32 [count, dim / 32], for a binary index; codes, uint8 [count, M], for a pq8 index."""
    hdr = read_header(path)
    if hdr["dtype"] == PQ:
        m = hdr["pq"]["m"]
        return np.fromfile(path, np.uint8, hdr["count"] * m, offset=hdr["data_off"]).reshape(hdr["count"], m)
    if hdr["dtype"] == BIN:
        w = hdr["dim"] // 32
        return np.fromfile(path, "<u4", hdr["count"] * w, offset=hdr["data_off"]).astype(np.uint32).reshape(hdr["count"], w)
    dt = np.uint8 if hdr["dtype"] == FP8 else np.uint16
    n = stored_rows(hdr)
    return np.fromfile(path, dt, n * hdr["dim"], offset=hdr["data_off"]).reshape(n, hdr["dim"])


def read_ivf(path: str) -> dict:
    """The tables of an IVF index, validated: ``centroids`` (bf16 bits uint16 [nlist, dim]), ``list_off`` int32
    [nlist + 1], ``list_tiles`` int32 [tiles], ``rowid`` int32 [capacity], and what follows from them: ``pos``
    int32 [count] (the stored row of each id) and ``list_of`` int32 [count] (its list). A ValueError names the
    first inconsistency: offsets that do not rise from 0 to the tile count, a tile id out of range or in two
    lists, ids that are not each present once, a live padding row or a list whose ids do not ascend."""
    hdr = read_header(path)
    if "ivf" not in hdr:
        raise ValueError(f"{path}: not an IVF index (version 5 holds the lists)")
    ivf, n, cap, dim = hdr["ivf"], hdr["count"], hdr["capacity"], hdr["dim"]
    nlist, ntile = ivf["nlist"], cap // TILE
    cent = np.fromfile(path, "<u2", nlist * dim, offset=ivf["centroids_off"]).astype(np.uint16).reshape(nlist, dim)
    off = np.fromfile(path, "<i4", nlist + 1, offset=ivf["list_off_off"]).astype(np.int32)
    tiles = np.fromfile(path, "<i4", ntile, offset=ivf["list_tiles_off"]).astype(np.int32)
    rowid = np.fromfile(path, "<i4", cap, offset=ivf["rowid_off"]).astype(np.int32)
    if not np.isfinite(bf16_to_f32(cent)).all():
        raise ValueError(f"{path}: an ivf centroid is not finite")
    if off[0] != 0 or off[-1] != ntile or (np.diff(off) < 0).any():
        raise ValueError(f"{path}: ivf list_off does not rise from 0 to the {ntile} tiles")
    if tiles.size and (tiles.min() < 0 or tiles.max() >= ntile):
        raise ValueError(f"{path}: an ivf list_tiles entry is outside [0, {ntile})")
    if np.unique(tiles).size != ntile:
        raise ValueError(f"{path}: ivf list_tiles names a tile twice (every tile belongs to exactly one list)")
    real = rowid >= 0
    if (rowid < -1).any() or (rowid >= n).any() or int(real.sum()) != n or np.unique(rowid[real]).size != n:
        raise ValueError(f"{path}: ivf rowid is not a permutation of the {n} ids over the stored rows (-1 on padding)")
    if read_live(path)[~real].any():
        raise ValueError(f"{path}: a padding row of the IVF index is live")
    tile_list = np.empty(ntile, np.int32)
    tile_list[tiles] = np.repeat(np.arange(nlist, dtype=np.int32), np.diff(off))
    seq = rowid.reshape(ntile, TILE)[tiles].reshape(-1)   # the stored rows in list order
    lst = np.repeat(tile_list[tiles], TILE)
    keep = seq >= 0
    ids, lst = seq[keep], lst[keep]
    if ((np.diff(ids) <= 0) & (np.diff(lst) == 0)).any():
        raise ValueError(f"{path}: the ids of an ivf list do not ascend in stored order")
    pos = np.empty(n, np.int32)
    pos[rowid[real]] = np.flatnonzero(real)
    return {"centroids": cent, "list_off": off, "list_tiles": tiles, "rowid": rowid, "pos": pos,
            "list_of": tile_list[pos // TILE], **{k: ivf[k] for k in ("nlist", "nprobe", "seed", "iters")}}


def ivf_facts(hdr: dict, t: dict) -> dict:
    """What ``describe()`` and ``hipzap info`` say about the lists."""
    sizes = np.bincount(t["list_of"], minlength=t["nlist"])
    return {"nlist": int(t["nlist"]), "nprobe": int(t["nprobe"]), "seed": int(t["seed"]), "iters": int(t["iters"]),
            "empty_lists": int((sizes == 0).sum()), "largest_list": int(sizes.max()), "tiles": int(hdr["capacity"] // TILE),
            "padding_rows": int(hdr["capacity"] - hdr["count"])}


def read_scales(path: str) -> np.ndarray:
    """The row scales of an fp8 index, float32 [count] ([capacity], in stored order, for an IVF index)."""
    hdr = read_header(path)
    if hdr["dtype"] != FP8:
        raise ValueError(f"{path}: a {hdr['dtype']} index has no scales")
    return np.fromfile(path, "<f4", stored_rows(hdr), offset=hdr["scales_off"]).astype(np.float32)


def read_codebook(path: str) -> np.ndarray:
    """The codebook of a pq8 index, float32 [M, 256, dim / M]."""
    hdr = read_header(path)
    if hdr["dtype"] != PQ:
        raise ValueError(f"{path}: a {hdr['dtype']} index has no codebook")
    blk = hdr["pq"]
    return np.fromfile(path, "<f4", PQ_KSUB * hdr["dim"], offset=blk["codebook_off"]).astype(np.float32) \
        .reshape(blk["m"], PQ_KSUB, blk["dsub"])


def read_rescore_rows(path: str) -> np.ndarray:
    """The rescore block of a version-4 or version-7 index: bf16 bit patterns, uint16 [count, dim], row ``i`` the
    vector of id ``i`` (also in an IVF index, whose other blocks are in stored order)."""
    hdr = read_header(path)
    if "rescore_off" not in hdr:
        raise ValueError(f"{path}: a {hdr['dtype']} index without rescore rows (version 4 holds them)")
    return np.fromfile(path, "<u2", hdr["count"] * hdr["dim"], offset=hdr["rescore_off"]) \
        .astype(np.uint16).reshape(hdr["count"], hdr["dim"])


def rescore_ref(rrows, q, ids, k: int):
    """The oracle's second stage: query ``q`` ([D]) against the candidates ``ids`` (stage one's, -1 in unused
    slots) of ``rrows`` (the bf16 rescore rows widened to fp32, [N, D]) in fp64 -> (scores float64 [k], ids int32
    [k]) under the order rule."""
    ids = np.asarray(ids)
    ids = ids[ids >= 0]
    s = (np.asarray(rrows[ids], np.float64) * np.asarray(q, np.float64)[None, :]).sum(axis=1) + 0.0
    order = np.lexsort((ids, -s))[:k]  # higher score first, then the lower id
    scores, out = np.full(k, -np.inf), np.full(k, -1, np.int32)
    scores[:order.size], out[:order.size] = s[order], ids[order]
    return scores, out


def search_ref(corpus, q, k: int, allow=None, scales=None):
    """The oracle: ``corpus`` (the bf16 rows widened to fp32, [N, D]) against ``q`` (fp32 [Q, D]) in fp64
    -> (scores float64 [Q, k], ids int32 [Q, k]) under the order rule. Each score is one row's own sum, so
    equal rows give equal scores wherever they stand. ``allow`` (bool [N] or [Q, N]): only these rows may be
    returned, under their own ids; the slots past the allowed rows hold id -1, score -inf. ``scales`` ([N],
    an fp8 index): row r's score is ``scales[r]`` times its sum over the decoded codes."""
    c = np.asarray(corpus, np.float64)
    q = np.asarray(q, np.float64)
    if q.ndim == 1:
        q = q[None]
    n = c.shape[0]
    if allow is not None:
        allow = np.asarray(allow, bool)
        if allow.shape not in ((n,), (q.shape[0], n)):
            raise ValueError(f"allow must be bool [{n}] or [{q.shape[0]}, {n}], got {list(allow.shape)}")
    scores = np.full((q.shape[0], k), -np.inf)
    ids = np.full((q.shape[0], k), -1, np.int32)
    for i, row in enumerate(q):
        s = (c * row[None, :]).sum(axis=1)
        if scales is not None:
            s = s * np.asarray(scales, np.float64)
        s = s + 0.0  # -0.0 + 0.0 = +0.0
        if allow is None:
            order = np.argsort(-s, kind="stable")[:k]  # stable: equal scores keep ascending ids
        else:
            rows = np.flatnonzero(allow if allow.ndim == 1 else allow[i])
            order = rows[np.argsort(-s[rows], kind="stable")[:k]]
        scores[i, :order.size] = s[order]
        ids[i, :order.size] = order
    return scores, ids


def split3(q):
    """The batch scan's split of fp32 values (csrc/hipzap.h HZ_K_SEARCH_XSCAN, "THE SPLIT") -> (h', m', l'), three fp32
    arrays of bf16 values: ``h`` keeps the top 16 bits of ``x``, ``m`` the top 16 bits of ``x - h``, ``l = (x - h) -
    m`` (both differences are exact in fp32); then every term whose exponent field is zero becomes a zero of its own
    sign. ``h' + m' + l'`` is the effective query ``x'``: equal to ``x`` unless a term is below 2^-126."""
    x = np.ascontiguousarray(q, np.float32)

    def top(a):
        return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)

    def term(a):
        b = a.view(np.uint32)
        return np.where(b & np.uint32(0x7F800000), b, b & np.uint32(0x80000000)).astype(np.uint32).view(np.float32)
    h = top(x)
    r1 = x - h
    m = top(r1)
    return term(h), term(m), term(r1 - m)


def batch_candidates(k: int, candidates=None) -> int:
    """``search_batch(candidates=...)`` -> R, the stage-one candidates per query: ``None`` means
    ``min(MAX_K, max(4 k, k + 32))``, else an integer in k..MAX_K."""
    if candidates is None:
        return min(MAX_K, max(4 * k, k + 32))
    if not _is_int(candidates) or not k <= candidates <= MAX_K:
        raise ValueError(f"candidates must be None or an integer in k..{MAX_K}, got {candidates!r} with k = {k}")
    return int(candidates)


COSINE_RMAX = 1.0 + 2.0 ** -7  # the most a row of a cosine index can measure: normalised in fp32, then rounded to bf16


def batch_slack(q, metric: str):
    """E of the certificate per query (float64 [Q]), or None where no bound on the rows is known (an ``ip`` index).
    A row outside the candidates has a stage-one score of at most s_R; its score in ``search`` is then at most
    s_R + E with E = (beta(3D) + gamma(D)) * B: beta(n) = n 2^-23 / (1 - n 2^-23) bounds the batch scan's error
    (csrc/hipzap.h), gamma(D) = D 2^-24 / (1 - D 2^-24) the fp32 scan's, and B = ||q||_2 * rmax bounds
    sum |q_i r_i| for both (|x'_i| <= |x_i|). The terms the split flushes (each below 2^-126) add at most
    3 * 2^-126 * sqrt(D) * rmax, which is included."""
    if metric != "cosine":
        return None
    q64 = np.asarray(q, np.float64)
    d = q64.shape[1]
    beta = 3 * d * 2.0 ** -23 / (1 - 3 * d * 2.0 ** -23)
    gamma = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
    return (beta + gamma) * np.sqrt((q64 * q64).sum(axis=1)) * COSINE_RMAX + 3 * 2.0 ** -126 * np.sqrt(d) * COSINE_RMAX


def batch_certain(s_last, t_k, slack):
    """The certificate: ``s_last`` [Q] the stage-one score of each query's R-th candidate (-inf: fewer than R rows
    passed, so every passing row was a candidate), ``t_k`` [Q] the k-th returned score, ``slack`` from
    :func:`batch_slack` -> bool [Q]: the answer is proven equal to ``search``'s. Without a slack only the first
    clause applies."""
    s_last, t_k = np.asarray(s_last, np.float64), np.asarray(t_k, np.float64)
    certain = np.isneginf(s_last)
    if slack is not None:
        certain = certain | (s_last + slack < t_k)
    return certain


def check_queries(q, dim: int) -> np.ndarray:
    q = np.asarray(q)
    if q.ndim == 1:
        q = q[None]
    if q.ndim != 2 or q.shape[1] != dim:
        raise ValueError(f"query vectors must be [Q, {dim}], got {list(q.shape)}")
    q = np.ascontiguousarray(q, np.float32)
    if not np.isfinite(q).all():
        raise ValueError("a query vector has a non-finite value")
    return q


def check_k(k) -> int:
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in 1..{MAX_K}, got {k!r}")
    return int(k)


def normalize_rows(q: np.ndarray) -> np.ndarray:
    """q / max(||q||, 1e-12) per row in fp32 (what a cosine index expects of its queries)."""
    q = np.asarray(q, np.float32)
    norm = np.sqrt((q * q).sum(axis=1, dtype=np.float32), dtype=np.float32)
    return q / np.maximum(norm, np.float32(1e-12))[:, None]


def check_filter(filter, nq: int):
    """``filter`` -> uint32 [nq, 2] of {mask, value} per query, or None: ``(mask, value)`` for every query,
    or a sequence of ``nq`` such pairs; integers in 0..2^32-1."""
    if filter is None:
        return None

    def is_int(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, bool)
    f = list(filter) if not isinstance(filter, np.ndarray) else filter.tolist()
    if len(f) == 2 and is_int(f[0]) and is_int(f[1]):
        f = [f] * nq
    if len(f) != nq:
        raise ValueError(f"filter must be (mask, value) or {nq} such pairs, got {len(f)}")
    out = np.empty((nq, 2), np.uint32)
    for i, pair in enumerate(f):
        pair = list(pair) if isinstance(pair, (list, tuple, np.ndarray)) else [pair]
        if len(pair) != 2 or not all(is_int(x) and 0 <= x <= 0xFFFFFFFF for x in pair):
            raise ValueError(f"filter {i}: mask and value must be integers in 0..2^32-1, got {pair!r}")
        out[i] = pair
    return out


class _QRows:
    """What ``add`` hands a backend's ``_append`` on an fp8 index: the codes and their row scales; on an index
    with rescore rows also ``rescore``, the bf16 bit patterns of the same input."""

    def __init__(self, codes, scales, rescore=None):
        self.codes, self.scales, self.shape = np.ascontiguousarray(codes), np.ascontiguousarray(scales, np.float32), codes.shape
        self.rescore = None if rescore is None else np.ascontiguousarray(rescore, np.uint16)


class _BRows:
    """What ``add`` hands a backend's ``_append`` on a binary index: the sign-bit words; on an index with rescore
    rows also ``rescore``, the bf16 bit patterns of the same input. ``shape`` is [n, dim]."""

    def __init__(self, words, dim: int, rescore=None):
        self.words = np.ascontiguousarray(words, np.uint32)
        self.shape = (self.words.shape[0], dim)
        self.rescore = None if rescore is None else np.ascontiguousarray(rescore, np.uint16)


class _PRows:
    """What ``add`` hands a backend's ``_append`` on a pq8 index: the codes (encoded against the index's codebook); on
    an index with rescore rows also ``rescore``, the bf16 bit patterns of the same input. ``shape`` is [n, dim]."""

    def __init__(self, codes, dim: int, rescore=None):
        self.codes = np.ascontiguousarray(codes, np.uint8)
        self.shape = (self.codes.shape[0], dim)
        self.rescore = None if rescore is None else np.ascontiguousarray(rescore, np.uint16)


class _Base:
    """What both backends share: the header, the argument checks of the mutators and ``save``. A backend
    provides ``_append(bits, tags, publish)`` (which calls ``publish(first id)`` before searches may run again), ``_kill(ids) -> int``, ``_retag(ids, tags)`` and ``_state() -> (bits,
    tags, live)``. On an fp8 index ``bits`` is a ``_QRows`` and ``_state`` returns ``(codes, tags, live, scales)``,
    on one with rescore rows ``(codes, tags, live, scales, rescore rows)``."""

    def __init__(self, path: str):
        self.path = path
        self.header = read_header(path)
        self.dim, self.count, self.metric = self.header["dim"], self.header["count"], self.header["metric"]
        self.labels = self.header.get("labels")
        self.dtype = self.header["dtype"]
        self.rescore = "rescore_off" in self.header  # a version-4 file: bf16 rows for a second stage
        self.ivf = read_ivf(path) if "ivf" in self.header else None  # the validated tables of a version-5 file
        self.codebook = read_codebook(path) if self.dtype == PQ else None  # what add encodes against
        if self.dtype == BIN:
            self.version = VERSION9 if self.rescore else VERSION8
        elif self.dtype == PQ:
            self.version = VERSION11 if self.rescore else VERSION10
        elif self.ivf:
            self.version = VERSION5 if self.dtype != FP8 else VERSION7 if self.rescore else VERSION6
        else:
            self.version = (VERSION4 if self.rescore else VERSION3 if self.dtype == FP8
                            else VERSION2 if "tags_off" in self.header else VERSION)
        self.nprobe = self.ivf["nprobe"] if self.ivf else None  # what search(nprobe=None) scans; settable
        self._mut = threading.Lock()  # one mutator at a time

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check_ids(self, ids) -> np.ndarray:
        a = np.atleast_1d(np.asarray(ids))
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError(f"ids must be a list of integers, got {a.dtype} {list(a.shape)}")
        bad = a[(a < 0) | (a >= self.count)] if a.size else a
        if bad.size:
            raise ValueError(f"id {int(bad[0])} is outside [0, {self.count})")
        return np.ascontiguousarray(a.astype(np.int32))

    def _refine(self, refine, k: int) -> int:
        """``search(refine=...)`` -> the R of the two-stage search, 0 for a one-stage search. On an index with
        rescore rows ``None`` means ``MAX_K`` (a cluster of ~100 near neighbours loses its order under fp8,
        DESIGN.md 4n, and 128 is the most the merge supports), ``0`` turns rescoring off and an integer in
        ``[k, MAX_K]`` is taken as given; on any other index only ``None`` and ``0`` are accepted."""
        if refine is None:
            return MAX_K if self.rescore else 0
        if isinstance(refine, (int, np.integer)) and not isinstance(refine, bool):
            if refine == 0 or (self.rescore and k <= refine <= MAX_K):
                return int(refine)
        wants = f"None, 0 or an integer in [k, {MAX_K}]" if self.rescore else "None or 0 (the index has no rescore rows)"
        raise ValueError(f"refine must be {wants}, got {refine!r} with k = {k} on a {self.dtype} index of version "
                         f"{self.version}")

    def _nprobe(self, nprobe, refine=None) -> int:
        """``search(nprobe=...)`` -> the lists to scan, 0 for every list (and for an index without lists). On an
        IVF index ``None`` means ``self.nprobe`` (the header's default unless set), ``"all"`` or a value from
        ``nlist`` up scans every list, which is exact; anything else must be an integer in 1..min(nlist, MAX_K)."""
        if self.ivf is None:
            if nprobe is not None:
                raise ValueError(f"nprobe={nprobe!r} needs an IVF index (write_index(ivf=...)), this one is "
                                 f"{self._bin_name()}version {self.version}")
            return 0
        if refine not in (None, 0) and not self.rescore:
            raise ValueError(f"refine={refine!r}: an IVF index has no rescore rows unless it is a version-7 file "
                             f"(convert_index(..., 'fp8', rescore=True)), this one is version {self.version}")
        nlist = self.ivf["nlist"]
        if nprobe is None:
            nprobe = self.nprobe
        if isinstance(nprobe, str) and nprobe == "all":
            return 0
        if not _is_int(nprobe) or nprobe < 1 or (nprobe > MAX_K and nprobe < nlist):
            raise ValueError(f"nprobe must be an integer in 1..{min(nlist, MAX_K)}, 'all' or at least nlist = {nlist}, "
                             f"got {nprobe!r}")
        return 0 if nprobe >= nlist else int(nprobe)

    def _bin_name(self) -> str:
        """"a bin_sign index of " on a binary index, "a pq8 index of " on a pq8 one (the by-name refusals), else nothing."""
        return f"a {self.dtype} index of " if self.dtype in (BIN, PQ) else ""

    def _check_probes(self, q, nprobe):
        if self.ivf is None:
            raise ValueError(f"probes needs an IVF index (write_index(ivf=...)), this one is {self._bin_name()}version "
                             f"{self.version}")
        if not _is_int(nprobe) or not 1 <= nprobe <= min(self.ivf["nlist"], MAX_K):
            raise ValueError(f"nprobe must be an integer in 1..{min(self.ivf['nlist'], MAX_K)}, got {nprobe!r}")
        return check_queries(q, self.dim), int(nprobe)

    def _check_neighbors(self, ids, k):
        """The refusals of :meth:`neighbors` that both backends share -> (ids int32 [n], k)."""
        if self.dtype in (FP8, BIN, PQ) or self.ivf is not None:
            what = ("an fp8 IVF index" if self.dtype == FP8 else "an IVF index") if self.ivf is not None else \
                f"a {self.dtype} index" if self.dtype in (BIN, PQ) else f"an {FP8} index"
            raise ValueError(f"neighbors is built for plain bf16 indexes (versions 1 and 2): this one is {what} of version "
                             f"{self.version}")
        if self.dim % 32:
            raise ValueError(f"neighbors needs dim % 32 == 0 (one MFMA step is 32 columns), got dim = {self.dim}")
        return self._check_ids(ids), check_k(k)

    def _check_batch(self, k, candidates):
        """The refusals of :meth:`search_batch` that both backends share -> (k, R)."""
        if self.dtype in (FP8, BIN, PQ) or self.ivf is not None:
            what = ("an fp8 IVF index" if self.dtype == FP8 else "an IVF index") if self.ivf is not None else \
                f"a {self.dtype} index" if self.dtype in (BIN, PQ) else f"an {FP8} index"
            raise ValueError(f"search_batch is built for plain bf16 indexes (versions 1 and 2): this one is {what} of "
                             f"version {self.version}")
        if self.dim % 32:
            raise ValueError(f"search_batch needs dim % 32 == 0 (one MFMA step is 32 columns), got dim = {self.dim}")
        k = check_k(k)
        return k, batch_candidates(k, candidates)

    def _check_cluster_index(self):
        """:meth:`cluster` is built for plain bf16 indexes with ``dim % 32 == 0``."""
        if self.dtype in (FP8, BIN, PQ) or self.ivf is not None:
            what = ("an fp8 IVF index" if self.dtype == FP8 else "an IVF index") if self.ivf is not None else \
                f"a {self.dtype} index" if self.dtype in (BIN, PQ) else f"an {FP8} index"
            raise ValueError(f"cluster is built for plain bf16 indexes (versions 1 and 2): this one is {what} of version "
                             f"{self.version}")
        if self.dim % 32:
            raise ValueError(f"cluster needs dim % 32 == 0 (one MFMA step is 32 columns), got dim = {self.dim}")

    def _check_cluster(self, nlist, iters, seed, init, nlive: int):
        """The argument refusals of :meth:`cluster` that both backends share -> init as fp32 or None."""
        if not _is_int(nlist) or not 1 <= nlist <= min(nlive, IVF_MAX_LISTS):
            raise ValueError(f"nlist must be an integer in 1..min(live rows, {IVF_MAX_LISTS}) = 1..{min(nlive, IVF_MAX_LISTS)}, "
                             f"got {nlist!r}")
        if not _is_int(iters) or iters < 0:
            raise ValueError(f"iters must be an integer >= 0, got {iters!r}")
        if not _is_int(seed) or seed < 0:
            raise ValueError(f"seed must be an integer >= 0, got {seed!r}")
        return None if init is None else check_init(init, int(nlist), self.dim)

    def cluster(self, nlist: int, *, iters: int = 10, seed: int = 0, init=None, ctx: int | None = None):
        """k-means over the live rows -> (centroid bf16 bits uint16 [nlist, dim], the cluster of every row int32 [count],
        its score float32 [count]); a deleted row gets -1 / -inf. :func:`ivf_kmeans`'s algorithm: the same sample draw
        and the same first centroids (``nlist`` distinct sample rows, or ``init``), both taken over the live rows;
        assignment by the largest inner product with the bf16 centroids, the lowest index among equals; a centroid
        is its members' mean (``cosine``: divided by its norm) and keeps its value when it has none. The training
        assignments cover the sample only, the last one every live row. On :class:`Index` both steps run on the
        GPU; :class:`RefIndex` scores and averages in fp64. ``ctx`` is the GPU backend's context."""
        self._check_cluster_index()
        live = self._live_now()
        ids = np.flatnonzero(live)
        init = self._check_cluster(nlist, iters, seed, init, ids.size)
        nlist = int(nlist)
        rng = np.random.default_rng(seed)
        n = ids.size
        m = min(n, IVF_SAMPLE * nlist)
        sample = ids[np.sort(rng.choice(n, m, replace=False))] if m < n else ids
        first = sample[np.sort(rng.choice(m, nlist, replace=False))]
        bits = self._cluster_rows(first) if init is None else to_bf16(init)
        take = np.zeros(self.count, bool)
        take[sample] = True
        trace = None
        with self._cluster_hold(ctx) as ctx:  # one context for the whole job: its buffers are allocated once
            for _ in range(int(iters)):
                a = self._cluster_assign(bits, take, ctx)[0]
                order = np.argsort(a[sample], kind="stable")  # ascending ids inside a cluster, as in ivf_kmeans
                seg_off = np.concatenate([[0], np.cumsum(np.bincount(a[sample], minlength=nlist))]).astype(np.int32)
                bits, c32 = self._cluster_update(np.ascontiguousarray(sample[order], np.int32), seg_off, bits, ctx)
                trace = (a, c32)
            assign, score = self._cluster_assign(bits, live, ctx)
        self._cluster_trace = trace  # the last training assignment and the fp32 centroids it gave (tests)
        return bits, assign, score

    @contextlib.contextmanager
    def _cluster_hold(self, ctx):
        yield ctx

    def knn_graph(self, k: int = 10, *, block: int = NEIGHBORS_BLOCK):
        """The kNN graph of the index: :meth:`neighbors` of every live row (itself excluded), ``block`` rows a pass
        -> (ids int32 [count, k], scores float32 [count, k]). A deleted row's lists hold -1 / -inf."""
        if not _is_int(block) or block < 1:
            raise ValueError(f"block must be a positive integer, got {block!r}")
        self._check_neighbors([], k)
        live = np.flatnonzero(self._live_now())
        ids = np.full((self.count, k), -1, np.int32)
        scores = np.full((self.count, k), -np.inf, np.float32)
        for a in range(0, live.size, block):
            part = live[a:a + block]
            scores[part], ids[part] = self.neighbors(part, k)
        return ids, scores

    def add(self, vectors, tags=None, labels=None, *, encoder: str = "cpu") -> np.ndarray:
        """Append rows (fp32 [n, dim], through :func:`prepare_rows` or, on an fp8 index, :func:`prepare_rows_fp8`:
        the bits ``write_index`` would store) -> their ids, int32 [n]. ``tags``: uint32 [n], default 0.
        ``labels``: required iff the index has labels. ``encoder`` (a pq8 index only): the backend of
        :func:`pq_encode` that encodes the new rows against the index's codebook, ``"gpu"`` on the index's device."""
        _check_pq_backend(encoder, "encoder")
        if encoder != "cpu" and self.dtype != PQ:
            raise ValueError(f"encoder={encoder!r} goes with a pq8 index (its rows are encoded against a codebook); this "
                             f"index holds {self.dtype} rows")
        if self.ivf is not None:
            raise ValueError("IVF indexes do not take add yet: write a new index with write_index(ivf=...)")
        if self.dtype == FP8:
            bits = _QRows(*prepare_rows_fp8(vectors, self.metric),
                          rescore=prepare_rows(vectors, self.metric) if self.rescore else None)
        elif self.dtype == BIN:  # binarised here, on the host: the same words write_index stores
            bits = _BRows(prepare_rows_bin(vectors, self.metric), np.asarray(vectors).shape[1],
                          rescore=prepare_rows(vectors, self.metric) if self.rescore else None)
        elif self.dtype == PQ:  # encoded here, on the host, against the file's codebook: the bytes write_index stores
            rbits = prepare_rows(vectors, self.metric)
            if rbits.shape[1] != self.dim:
                raise ValueError(f"vectors must be [N, {self.dim}], got {list(rbits.shape)}")
            bits = _PRows(pq_encode(bf16_to_f32(rbits), self.codebook, backend=encoder, device=getattr(self, "device", 0)),
                          self.dim, rescore=rbits if self.rescore else None)
        else:
            bits = prepare_rows(vectors, self.metric)
        n = bits.shape[0]
        if bits.shape[1] != self.dim:
            raise ValueError(f"vectors must be [N, {self.dim}], got {list(bits.shape)}")
        if (labels is not None) != (self.labels is not None):
            raise ValueError("labels are required: the index has labels" if labels is None
                             else "the index has no labels")
        if labels is not None:
            labels = [str(x) for x in labels]
            if len(labels) != n:
                raise ValueError(f"{len(labels)} labels for {n} rows")
        tags = np.zeros(n, np.uint32) if tags is None else check_tags(tags, n)
        with self._mut:
            if self.count + n >= 2 ** 31:
                raise ValueError("count must stay below 2^31")

            def publish(first):  # runs while searches are still excluded: no search sees an id without its label
                if labels is not None:
                    self.labels = list(self.labels) + labels
                self.count = first + n
                self.header["count"] = self.count
            first = self._append(bits, tags, publish)
        return np.arange(first, first + n, dtype=np.int32)

    def delete(self, ids) -> int:
        """Hide rows for good -> how many were live until now. An id outside [0, count) is a ValueError."""
        with self._mut:
            return int(self._kill(self._check_ids(ids)))

    def set_tags(self, ids, tags) -> None:
        with self._mut:
            ids = self._check_ids(ids)
            self._retag(ids, check_tags(tags, ids.size))

    def save(self, path: str | None = None, compact: bool = False) -> dict:
        """Write the index as it stands (atomic: a temporary file, then a rename) -> the JSON header.
        ``compact=False`` keeps ids and tombstones; ``compact=True`` drops the dead rows and renumbers the
        rest in order. Version 1 when every row is live and every tag is 0, else version 2; an fp8 index is
        version 3 with or without tags and bitmap under the same rule, and version 4 when it has rescore rows."""
        if self.ivf is not None and compact:
            raise ValueError("IVF indexes do not take save(compact=True) yet: ids would change with the lists' layout")
        with self._mut:
            bits, tags, live, *rest = self._state()
            scales = rest[0] if rest else None
            rrows = rest[1] if len(rest) > 1 else None
            if self.ivf is not None:  # stored order, as it was read: the same version again, the same tables
                hdr = {"dim": self.dim, "count": self.count, "dtype": self.dtype, "metric": self.metric,
                       "model": self.header.get("model", ""), "embed": self.header.get("embed")}
                if self.labels is not None:
                    hdr["labels"] = list(self.labels)
                return _write_file(path or self.path, hdr, np.ascontiguousarray(bits), tags, live, scales=scales,
                                   rescore=rrows, ivf=self.ivf)
            labels = self.labels
            if compact:
                if not live.any():
                    raise ValueError("no live row to save")
                bits, tags = bits[live], tags[live]
                scales = scales[live] if scales is not None else None
                rrows = rrows[live] if rrows is not None else None
                labels = [x for x, keep in zip(labels, live) if keep] if labels is not None else None
                live = np.ones(bits.shape[0], bool)
            hdr = {"dim": self.dim, "count": int(bits.shape[0]), "dtype": self.dtype, "metric": self.metric,
                   "model": self.header.get("model", ""), "embed": self.header.get("embed")}
            if labels is not None:
                hdr["labels"] = list(labels)
            plain = bool(live.all()) and not tags.any()
            return _write_file(path or self.path, hdr, np.ascontiguousarray(bits), None if plain else tags,
                               None if plain else live, self.capacity(), scales=scales, rescore=rrows, pq=self.codebook)


class RefIndex(_Base):
    """The index on the host: :func:`search_ref` over the rows (the CPU backend's implementation and the
    oracle of the GPU one)."""
    backend = "cpu"

    def __init__(self, path: str, reserve: int = 0):
        super().__init__(path)
        self._bits = read_rows(path)
        fp8 = self.dtype == FP8
        self._rows = None if self.dtype in (BIN, PQ) else e4m3_to_f32(self._bits) if fp8 else bf16_to_f32(self._bits)
        self.scales = read_scales(path) if fp8 else None
        self._rbits = read_rescore_rows(path) if self.rescore else None
        self._rrows = bf16_to_f32(self._rbits) if self.rescore else None
        self._tags, self._live = read_tags(path), read_live(path)
        self._cap = max(self.count, int(reserve), int(self.header.get("capacity", 0)))
        if self.ivf is not None:  # held by id, like every other index; _state() puts the stored order back
            pos = self.ivf["pos"]
            self._bits, self._rows, self._tags, self._live = self._bits[pos], self._rows[pos], self._tags[pos], self._live[pos]
            self.scales = self.scales[pos] if fp8 else None  # the rescore rows are in id order already
            self._cent = bf16_to_f32(self.ivf["centroids"])
            self._cap = int(self.header["capacity"])

    def allow(self, filt) -> np.ndarray:
        """bool [N] (no filter) or [Q, N]: the rows each query may return."""
        if filt is None:
            return self._live
        return self._live[None, :] & ((self._tags[None, :] & filt[:, :1]) == filt[:, 1:])

    def probes(self, q, nprobe: int) -> np.ndarray:
        """The ``nprobe`` lists nearest to each query, best first, int32 [Q, nprobe]: :func:`search_ref` over the
        centroids."""
        q, nprobe = self._check_probes(q, nprobe)
        return search_ref(self._cent, q, nprobe)[1]

    def search(self, q, k: int = 10, *, filter=None, refine=None, nprobe=None):
        """``refine`` (:meth:`_Base._refine`): R > 0 is the two-stage search -- ``search_ref(scales=...)`` at
        k = R, then those ids re-scored in fp64 over the widened bf16 rows (:func:`rescore_ref`). ``nprobe``
        (:meth:`_Base._nprobe`, an IVF index): only rows of the lists :meth:`probes` names may be returned."""
        q, k = check_queries(q, self.dim), check_k(k)
        filt = check_filter(filter, q.shape[0])
        lists = self._nprobe(nprobe, refine)
        R = self._refine(refine, k)
        with self._mut:  # the mutators replace the arrays one by one
            allow = None if filt is None and self._live.all() else self.allow(filt)
            if lists:
                near = (self.ivf["list_of"][None, :, None] == self.probes(q, lists)[:, None, :]).any(axis=2)  # [Q, N]
                allow = near if allow is None else near & allow
            if self.dtype == BIN:  # stage one: exact integer scores over the sign bits, ties by the lower id
                s, i = bin_search_ref(self._bits, binarize(q), self.dim, R or k, allow)
            elif self.dtype == PQ:  # stage one: the fp64 table, the exact inner product with the reconstructed rows
                s, i = pq_search_ref(self._bits, self.codebook, q, R or k, allow)
            else:
                s, i = search_ref(self._rows, q, R or k, allow, scales=self.scales)
            if R:
                two = [rescore_ref(self._rrows, q[a], i[a], k) for a in range(q.shape[0])]
                s, i = np.stack([t[0] for t in two]), np.stack([t[1] for t in two])
        return s.astype(np.float32), i

    def search_batch(self, q, k: int = 10, *, candidates=None, fallback: bool = True, ctx=None):
        """:meth:`Index.search_batch` on the host, its oracle: stage one is :func:`search_ref` in fp64 over the SPLIT
        query (:func:`split3`) at k = R, stage two :func:`rescore_ref` of those ids with the query itself, then the
        same certificate (:func:`batch_certain`) -> (scores float32 [Q, k], ids int32 [Q, k], certain bool [Q])."""
        k, R = self._check_batch(k, candidates)
        q = check_queries(q, self.dim)
        with self._mut:
            h, m, l = split3(q)
            eff = h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)
            s1, i1 = search_ref(self._rows, eff, R, None if self._live.all() else self._live)
            two = [rescore_ref(self._rows, q[a], i1[a], k) for a in range(q.shape[0])]
            s = np.stack([t[0] for t in two]) if two else np.zeros((0, k))
            i = np.stack([t[1] for t in two]) if two else np.zeros((0, k), np.int32)
        s, i = s.astype(np.float32), i.astype(np.int32)
        certain = batch_certain(s1[:, R - 1], s[:, k - 1], batch_slack(q, self.metric))
        if fallback and not certain.all():
            todo = np.flatnonzero(~certain)
            s[todo], i[todo] = self.search(q[todo], k)
            certain[:] = True
        return s, i, certain

    def neighbors(self, ids, k: int = 10, *, include_self: bool = False):
        """The ``k`` nearest live rows of each stored row ``ids`` names -> (scores float32 [n, k], ids int32 [n, k]):
        :func:`search_ref` in fp64 over the stored rows with ``allow`` = live and, unless ``include_self``, not the
        row itself. Other rows with the same bits stay and tie by id."""
        ids, k = self._check_neighbors(ids, k)
        with self._mut:
            dead = ids[~self._live[ids]]
            if dead.size:
                raise ValueError(f"id {int(dead[0])} is deleted")
            s = np.full((ids.size, k), -np.inf)
            out = np.full((ids.size, k), -1, np.int32)
            for a in range(0, ids.size, 256):  # the [n, N] allow matrix, 256 queries at a time
                part = ids[a:a + 256]
                allow = np.repeat(self._live[None, :], part.size, axis=0)
                if not include_self:
                    allow[np.arange(part.size), part] = False
                s[a:a + 256], out[a:a + 256] = search_ref(self._rows, self._rows[part], k, allow)
        return s.astype(np.float32), out

    def _live_now(self) -> np.ndarray:
        with self._mut:
            return self._live.copy()

    def _cluster_rows(self, ids):
        return self._bits[ids].copy()

    def _cluster_assign(self, bits, take, ctx=None):
        """fp64 scores over the bf16 centroids ``bits``; rows outside ``take`` get -1 / -inf."""
        cent = bf16_to_f32(bits).astype(np.float64)
        take = np.asarray(take, bool) & self._live
        out, score = np.full(self.count, -1, np.int32), np.full(self.count, -np.inf, np.float32)
        rows = np.flatnonzero(take)
        step = max(1, (1 << 22) // max(cent.shape[0], 1))
        for a in range(0, rows.size, step):
            part = rows[a:a + step]
            s = self._rows[part].astype(np.float64) @ cent.T
            best = np.argmax(s, axis=1)  # the lowest index among equals
            out[part], score[part] = best, s[np.arange(part.size), best]
        return out, score

    def _cluster_update(self, order, seg_off, bits, ctx=None):
        """fp64 means of the segments (``cosine``: divided by max(norm, 1e-12)); an empty segment keeps its bits."""
        bits = bits.copy()
        c32 = bf16_to_f32(bits)
        sizes = np.diff(seg_off)
        lists = np.flatnonzero(sizes)
        if lists.size:
            sums = np.add.reduceat(self._rows[order].astype(np.float64), seg_off[lists], axis=0)
            mean = sums / sizes[lists][:, None]
            if self.metric == "cosine":
                mean = mean / np.maximum(np.sqrt((mean * mean).sum(axis=1)), 1e-12)[:, None]
            c32[lists] = mean.astype(np.float32)
            bits[lists] = to_bf16(c32[lists])
        return bits, c32

    def _append(self, bits, tags, publish):
        first = self.count
        if self.dtype in (BIN, PQ):
            if self.rescore:
                self._rbits = np.concatenate([self._rbits, bits.rescore])
                self._rrows = np.concatenate([self._rrows, bf16_to_f32(bits.rescore)])
            self._bits = np.concatenate([self._bits, bits.words if self.dtype == BIN else bits.codes])
            self._tags = np.concatenate([self._tags, tags])
            self._live = np.concatenate([self._live, np.ones(bits.shape[0], bool)])
            while self._cap < self._bits.shape[0]:
                self._cap *= 2
            publish(first)
            return first
        if self.scales is not None:
            self.scales = np.concatenate([self.scales, bits.scales])
            if self.rescore:
                self._rbits = np.concatenate([self._rbits, bits.rescore])
                self._rrows = np.concatenate([self._rrows, bf16_to_f32(bits.rescore)])
            bits, new = bits.codes, e4m3_to_f32(bits.codes)
        else:
            new = bf16_to_f32(bits)
        self._bits = np.concatenate([self._bits, bits])
        self._rows = np.concatenate([self._rows, new])
        self._tags = np.concatenate([self._tags, tags])
        self._live = np.concatenate([self._live, np.ones(bits.shape[0], bool)])
        while self._cap < self._bits.shape[0]:
            self._cap *= 2
        publish(first)
        return first

    def _kill(self, ids):
        was = int(self._live.sum())
        self._live[ids] = False
        return was - int(self._live.sum())

    def _retag(self, ids, tags):
        self._tags[ids] = tags

    def _state(self):
        if self.ivf is not None:
            pos, cap = self.ivf["pos"], int(self.header["capacity"])
            bits, tags, live = np.zeros((cap, self.dim), self._bits.dtype), np.zeros(cap, np.uint32), np.zeros(cap, bool)
            bits[pos], tags[pos], live[pos] = self._bits, self._tags, self._live
            if self.scales is None:
                return bits, tags, live
            scales = np.ones(cap, np.float32)  # padding rows: code 0, scale 1, dead
            scales[pos] = self.scales
            return (bits, tags, live, scales, self._rbits) if self.rescore else (bits, tags, live, scales)
        if self.rescore:  # scales: None on a binary index
            return self._bits, self._tags, self._live, self.scales, self._rbits
        if self.scales is not None:
            return self._bits, self._tags, self._live, self.scales
        return self._bits, self._tags, self._live

    def capacity(self) -> int:
        return self._cap

    def describe(self) -> dict:
        return {"path": self.path, "backend": "cpu", **{k: v for k, v in self.header.items() if k != "labels"},
                "labels": self.labels is not None, "capacity": self._cap, "live": int(self._live.sum()),
                "tags": bool(self._tags.any()) or "tags_off" in self.header,
                **({"m": int(self.codebook.shape[0]), "dsub": int(self.codebook.shape[2]),
                    "codebook_bytes": int(self.codebook.nbytes)} if self.dtype == PQ else {}),
                **({"ivf": ivf_facts(self.header, self.ivf)} if self.ivf is not None else {})}

    def close(self) -> None:
        self._rows = None
        if self.dtype in (BIN, PQ):
            self._bits = None


class Index(_Base):
    """An open ``.hzidx`` on the GPU: the rows in device memory and ``contexts`` search contexts (each
    its own stream and buffers). :meth:`search` is thread-safe: a call takes a free context, or waits for
    one. Query batches above 16 rows are searched 16 at a time. ``reserve``: rows to allocate for (adds
    beyond the capacity grow it by doubling). A mutator takes every context before it calls native code,
    so a search sees the index entirely before or entirely after a mutation. ``rescore_rows`` (a version-4
    file): the bf16 rows of the second stage in ``"device"`` memory or in pinned ``"host"`` memory, which
    leaves the index at an fp8 index's device bytes."""
    backend = "gpu"

    def __init__(self, path: str, device: int = 0, contexts: int = 2, reserve: int = 0, rescore_rows: str = "device"):
        super().__init__(path)
        if rescore_rows not in ("device", "host"):
            raise ValueError(f"rescore_rows must be 'device' or 'host', got {rescore_rows!r}")
        from . import _native as N
        self._lib = N.lib()
        reserve = max(int(reserve), int(self.header.get("capacity", 0)))
        self.rescore_rows = rescore_rows if self.rescore else None
        self._h = self._lib.hz_index_open3(os.fsencode(path), int(device), int(contexts), reserve,
                                           int(rescore_rows == "host"))
        if not self._h:
            raise RuntimeError((self._lib.hz_index_last_error() or b"hz_index_open failed").decode())
        self.device, self.contexts = int(device), int(contexts)
        self._free: queue.Queue = queue.Queue()
        for c in range(self.contexts):
            self._free.put(c)

    def probes(self, q, nprobe: int, ctx: int | None = None) -> np.ndarray:
        """The ``nprobe`` lists nearest to each query, best first, int32 [Q, nprobe]: the coarse stage of a search
        alone (scan + merge over the centroids)."""
        q, nprobe = self._check_probes(q, nprobe)
        if self._h is None:
            raise RuntimeError("the index is closed")
        out = np.empty((q.shape[0], nprobe), np.int32)
        c = self._free.get() if ctx is None else ctx
        try:
            for a in range(0, q.shape[0], MAX_Q):
                part, o = q[a:a + MAX_Q], out[a:a + MAX_Q]
                rc = self._lib.hz_index_probes(self._h, c, part.ctypes.data, part.shape[0], nprobe, o.ctypes.data)
                if rc:
                    raise RuntimeError(f"hz_index_probes failed with code {rc}")
        finally:
            if ctx is None:
                self._free.put(c)
        return out

    def search(self, q, k: int = 10, ctx: int | None = None, *, filter=None, refine=None, nprobe=None):
        """fp32 queries [Q, dim] -> (scores float32 [Q, k], ids int32 [Q, k]), best first. ``filter``:
        ``(mask, value)`` for all queries or Q such pairs; a row passes iff ``(tag & mask) == value``.
        ``refine`` (an index with rescore rows): the candidates R that the fp8 scan hands the exact bf16
        second stage, ``None`` for 128, ``0`` for the fp8 answer alone (:meth:`_Base._refine`). ``nprobe`` (an
        IVF index): the lists each query scans, ``None`` for ``self.nprobe``, ``"all"`` for every list
        (:meth:`_Base._nprobe`)."""
        q, k = check_queries(q, self.dim), check_k(k)
        filt = check_filter(filter, q.shape[0])
        lists = self._nprobe(nprobe, refine)
        R = self._refine(refine, k)
        if self._h is None:
            raise RuntimeError("the index is closed")
        scores = np.empty((q.shape[0], k), np.float32)
        ids = np.empty((q.shape[0], k), np.int32)
        c = self._free.get() if ctx is None else ctx
        try:
            for a in range(0, q.shape[0], MAX_Q):
                part = q[a:a + MAX_Q]
                s, i = scores[a:a + MAX_Q], ids[a:a + MAX_Q]  # contiguous row ranges of the outputs
                f = None if filt is None else np.ascontiguousarray(filt[a:a + MAX_Q])
                rc = self._lib.hz_index_search3(self._h, c, part.ctypes.data, None if f is None else f.ctypes.data,
                                                part.shape[0], k, R, lists, s.ctypes.data, i.ctypes.data)
                if rc:
                    raise RuntimeError(f"hz_index_search failed with code {rc}")
        finally:
            if ctx is None:
                self._free.put(c)
        return scores, ids

    def search_batch(self, q, k: int = 10, *, candidates=None, fallback: bool = True, ctx: int | None = None):
        """Many fp32 queries at once -> (scores float32 [Q, k], ids int32 [Q, k], certain bool [Q]).
        Stage one scores every query against every live row with the bf16 MFMA -- each query split into three bf16
        terms that sum to it, so nothing is rounded away -- and keeps ``candidates`` rows per query (R: ``None`` for
        ``min(128, max(4 k, k + 32))``, else k..128); stage two re-scores those R with :meth:`search`'s own arithmetic
        and returns the best k. ``certain[q]``: the answer is PROVEN equal to ``search(q[None], k)`` in ids and score
        bits -- every row outside the candidates scored at most s_R in stage one, hence at most s_R + E in ``search``,
        and ``s_R + E < `` the k-th returned score (:func:`batch_slack`; E needs a bound on the rows, which only a
        ``cosine`` index has), or fewer than R rows passed. On an ``ip`` index only the second clause can certify.
        ``fallback``: the uncertain queries are re-run through :meth:`search` and are certain afterwards; with
        ``fallback=False`` they are returned as computed. A plain bf16 index with ``dim % 32 == 0``; Q above the
        per-call maximum is split here."""
        k, R = self._check_batch(k, candidates)
        q = check_queries(q, self.dim)
        if self._h is None:
            raise RuntimeError("the index is closed")
        nq = q.shape[0]
        scores, ids = np.empty((nq, k), np.float32), np.empty((nq, k), np.int32)
        last = np.empty(nq, np.float32)
        c = self._free.get() if ctx is None else ctx
        try:
            step = int(self._lib.hz_index_neighbors_max(self._h, 0))
            for a in range(0, nq, step):
                part = q[a:a + step]
                s, i, e = scores[a:a + step], ids[a:a + step], last[a:a + step]  # contiguous ranges of the outputs
                rc = self._lib.hz_index_search_batch(self._h, c, part.ctypes.data, part.shape[0], k, R, s.ctypes.data,
                                                     i.ctypes.data, e.ctypes.data)
                if rc in (-4, -5, -28, -44, -45):
                    raise ValueError((self._lib.hz_index_last_error() or b"").decode().replace("index: ", "", 1))
                if rc:
                    raise RuntimeError(f"hz_index_search_batch failed with code {rc}")
            certain = batch_certain(last, scores[:, k - 1] if nq else last, batch_slack(q, self.metric))
            if fallback and not certain.all():
                todo = np.flatnonzero(~certain)
                scores[todo], ids[todo] = self.search(q[todo], k, ctx=c)
                certain[:] = True
        finally:
            if ctx is None:
                self._free.put(c)
        return scores, ids, certain

    def neighbors(self, ids, k: int = 10, *, include_self: bool = False, ctx: int | None = None):
        """The ``k`` nearest live rows of each stored row ``ids`` names -> (scores float32 [n, k], ids int32 [n, k]),
        best first; the row itself is left out unless ``include_self`` (other rows with the same bits stay and tie
        by id). The rows never leave device memory: one pass is the bf16 MFMA self scan and its merge
        (DESIGN.md 4s), and ``n`` above the per-pass maximum is split here. A plain bf16 index with
        ``dim % 32 == 0``; an id outside [0, count) or a deleted id is a ValueError."""
        ids, k = self._check_neighbors(ids, k)
        if self._h is None:
            raise RuntimeError("the index is closed")
        scores = np.empty((ids.size, k), np.float32)
        out = np.empty((ids.size, k), np.int32)
        c = self._free.get() if ctx is None else ctx
        try:
            step = int(self._lib.hz_index_neighbors_max(self._h, 0))
            for a in range(0, ids.size, step):
                part = np.ascontiguousarray(ids[a:a + step])
                s, i = scores[a:a + step], out[a:a + step]  # contiguous row ranges of the outputs
                rc = self._lib.hz_index_neighbors(self._h, c, part.ctypes.data, part.size, k, int(not include_self),
                                                  s.ctypes.data, i.ctypes.data)
                if rc in (-4, -5, -20, -35, -36, -37):
                    raise ValueError((self._lib.hz_index_last_error() or b"").decode().replace("index: ", "", 1))
                if rc:
                    raise RuntimeError(f"hz_index_neighbors failed with code {rc}")
        finally:
            if ctx is None:
                self._free.put(c)
        return scores, out

    def _live_now(self) -> np.ndarray:
        with self._mut:
            n = self.count
            words = np.empty(-(-n // 32), np.uint32)
            self._exclusive(lambda: self._lib.hz_index_read_state(self._h, None, None, words.ctypes.data, n),
                            "hz_index_read_state")
        return unpack_live(words, n)

    def _cluster_rows(self, ids):
        return self._state()[0][ids].copy()

    @contextlib.contextmanager
    def _cluster_hold(self, ctx):
        """A free context (or ``ctx``) for the length of a clustering job."""
        if ctx is not None or self._h is None:
            yield ctx
            return
        c = self._free.get()
        try:
            yield c
        finally:
            self._free.put(c)

    def _cluster_call(self, ctx, call, what):
        if self._h is None:
            raise RuntimeError("the index is closed")
        c = self._free.get() if ctx is None else ctx
        try:
            rc = call(c)
        finally:
            if ctx is None:
                self._free.put(c)
        if rc in (-38, -39, -40, -41, -42, -43):
            raise ValueError((self._lib.hz_index_last_error() or b"").decode().replace("index: ", "", 1))
        if rc:
            raise RuntimeError(f"{what} failed with code {rc}")

    def _cluster_assign(self, bits, take, ctx=None):
        """HZ_K_SEARCH_ASSIGN over the index's rows against the bf16 centroids ``bits``; the native side ANDs ``take``
        (bool [count]) with the live bitmap."""
        bits = np.ascontiguousarray(bits, np.uint16)
        words = pack_live(take)
        out, score = np.empty(self.count, np.int32), np.empty(self.count, np.float32)
        self._cluster_call(ctx, lambda c: self._lib.hz_index_assign(self._h, c, bits.ctypes.data, bits.shape[0],
                                                                    words.ctypes.data, out.ctypes.data, score.ctypes.data),
                           "hz_index_assign")
        return out, score

    def _cluster_update(self, order, seg_off, bits, ctx=None):
        """HZ_K_SEARCH_CMEAN: the segments' means over ``bits`` -> (new bits, their fp32 values)."""
        bits = np.ascontiguousarray(bits, np.uint16).copy()
        c32 = bf16_to_f32(bits)
        order, seg_off = np.ascontiguousarray(order, np.int32), np.ascontiguousarray(seg_off, np.int32)
        self._cluster_call(ctx, lambda c: self._lib.hz_index_cmean(self._h, c, order.ctypes.data, order.size,
                                                                   seg_off.ctypes.data, bits.shape[0], bits.ctypes.data,
                                                                   c32.ctypes.data), "hz_index_cmean")
        return bits, c32

    def _exclusive(self, call, what):
        """Run a native mutation holding every context token (the caller holds the mutation lock, so no
        second mutator waits on a partial set)."""
        if self._h is None:
            raise RuntimeError("the index is closed")
        held = [self._free.get() for _ in range(self.contexts)]
        try:
            rc = call()
        finally:
            for c in held:
                self._free.put(c)
        if rc:
            raise RuntimeError(f"{what} failed with code {rc}")

    def _append(self, bits, tags, publish):
        first = C.c_longlong(-1)
        fp8, binary, pq = self.dtype == FP8, self.dtype == BIN, self.dtype == PQ
        if not fp8 and not binary and not pq:
            bits = np.ascontiguousarray(bits)

        def call():
            if pq and self.rescore:
                rc = self._lib.hz_index_add_pr(self._h, bits.codes.ctypes.data, bits.rescore.ctypes.data, bits.shape[0],
                                               tags.ctypes.data, C.byref(first))
            elif pq:
                rc = self._lib.hz_index_add_p(self._h, bits.codes.ctypes.data, bits.shape[0], tags.ctypes.data,
                                              C.byref(first))
            elif binary and self.rescore:
                rc = self._lib.hz_index_add_br(self._h, bits.words.ctypes.data, bits.rescore.ctypes.data, bits.shape[0],
                                               tags.ctypes.data, C.byref(first))
            elif binary:
                rc = self._lib.hz_index_add_b(self._h, bits.words.ctypes.data, bits.shape[0], tags.ctypes.data,
                                              C.byref(first))
            elif fp8 and self.rescore:
                rc = self._lib.hz_index_add_qr(self._h, bits.codes.ctypes.data, bits.scales.ctypes.data,
                                               bits.rescore.ctypes.data, bits.shape[0], tags.ctypes.data, C.byref(first))
            elif fp8:
                rc = self._lib.hz_index_add_q(self._h, bits.codes.ctypes.data, bits.scales.ctypes.data, bits.shape[0],
                                              tags.ctypes.data, C.byref(first))
            else:
                rc = self._lib.hz_index_add(self._h, bits.ctypes.data, bits.shape[0], tags.ctypes.data, C.byref(first))
            if rc == 0:
                publish(int(first.value))
            return rc
        self._exclusive(call, "hz_index_add")
        return int(first.value)

    def _kill(self, ids):
        gone = C.c_longlong(0)
        self._exclusive(lambda: self._lib.hz_index_delete(self._h, ids.ctypes.data, ids.size, C.byref(gone)),
                        "hz_index_delete")
        return int(gone.value)

    def _retag(self, ids, tags):
        self._exclusive(lambda: self._lib.hz_index_set_tags(self._h, ids.ctypes.data, tags.ctypes.data, ids.size),
                        "hz_index_set_tags")

    def _state(self):
        n = self.count if self.ivf is None else int(self.header["capacity"])  # an IVF index: the stored rows
        tags, words = np.empty(n, np.uint32), np.empty(-(-n // 32), np.uint32)
        if self.dtype in (BIN, PQ):
            if self.dtype == PQ:
                rows = np.empty((n, self.header["pq"]["m"]), np.uint8)
                self._exclusive(lambda: self._lib.hz_index_read_state_p(self._h, rows.ctypes.data, tags.ctypes.data,
                                                                        words.ctypes.data, n), "hz_index_read_state_p")
            else:
                rows = np.empty((n, self.dim // 32), np.uint32)
                self._exclusive(lambda: self._lib.hz_index_read_state_b(self._h, rows.ctypes.data, tags.ctypes.data,
                                                                        words.ctypes.data, n), "hz_index_read_state_b")
            if self.rescore:
                rrows = np.empty((n, self.dim), np.uint16)
                self._exclusive(lambda: self._lib.hz_index_read_rescore(self._h, rrows.ctypes.data, n),
                                "hz_index_read_rescore")
                return rows, tags, unpack_live(words, n), None, rrows
            return rows, tags, unpack_live(words, n)
        if self.dtype == FP8:
            codes, scales = np.empty((n, self.dim), np.uint8), np.empty(n, np.float32)
            self._exclusive(lambda: self._lib.hz_index_read_state_q(self._h, codes.ctypes.data, scales.ctypes.data,
                                                                    tags.ctypes.data, words.ctypes.data, n),
                            "hz_index_read_state_q")
            if self.rescore:
                nr = self.count  # an IVF index: its rescore rows are held by id, not in stored order
                rrows = np.empty((nr, self.dim), np.uint16)
                self._exclusive(lambda: self._lib.hz_index_read_rescore(self._h, rrows.ctypes.data, nr),
                                "hz_index_read_rescore")
                return codes, tags, unpack_live(words, n), scales, rrows
            return codes, tags, unpack_live(words, n), scales
        bits = np.empty((n, self.dim), np.uint16)
        self._exclusive(lambda: self._lib.hz_index_read_state(self._h, bits.ctypes.data, tags.ctypes.data,
                                                              words.ctypes.data, n), "hz_index_read_state")
        return bits, tags, unpack_live(words, n)

    def capacity(self) -> int:
        return self.describe()["capacity"]

    def describe(self) -> dict:
        out, more, pq = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
        self._lib.hz_index_describe(self._h, out)
        self._lib.hz_index_describe2(self._h, more)
        if self.dtype == PQ:
            self._lib.hz_index_describe4(self._h, pq)
        return {"path": self.path, "backend": "gpu", "device": self.device,
                **{k: v for k, v in self.header.items() if k != "labels"}, "labels": self.labels is not None,
                "contexts": int(out[3]), "tile_rows": int(out[4]), "programs": int(out[5]), "device_bytes": int(out[6]),
                "capacity": int(more[0]), "live": int(more[1]), "tags": bool(more[2]), "filtered": bool(more[3]),
                **({"rescore_rows": "host" if more[7] else "device"} if more[6] else {}),
                **({"m": int(pq[0]), "dsub": int(pq[1]), "codebook_bytes": int(pq[2]), "scan_span": int(pq[4])}
                   if self.dtype == PQ else {}),
                **({"ivf": ivf_facts(self.header, self.ivf)} if self.ivf is not None else {})}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.hz_index_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def open_index(path: str, backend: str = "gpu", device: int = 0, reserve: int = 0, rescore_rows: str = "device"):
    """``rescore_rows`` places a version-4 index's bf16 rows on the GPU backend; the CPU backend holds every row
    in host memory."""
    if backend == "gpu":
        return Index(path, device, reserve=reserve, rescore_rows=rescore_rows)
    return RefIndex(path, reserve)


def convert_index(src: str, dst: str, dtype: str = "fp8", rescore: bool = False, ivf=None, nprobe=None,
                  ivf_seed: int = 0, ivf_iters: int = 10, ivf_backend: str = "cpu", device: int = 0, pq_m=None,
                  pq_codebook=None, pq_seed: int = 0, pq_iters: int = 10, pq_backend: str = "cpu") -> dict:
    """Write the bf16 index ``src`` as ``dst`` in ``dtype`` -> the JSON header written. The stored rows are
    widened to fp32 and requantised as they stand (NOT renormalised: they are what the index searches);
    labels, model, embed, tags, the live bitmap and the capacity are carried over, so ids stay valid.
    ``rescore=True`` (fp8 only) keeps the stored bf16 rows as the rescore block: a version-4 file.
    An IVF ``src`` (version 5) keeps its lists, tables, centroids (bf16), ``nprobe``, ``seed`` and ``iters``:
    ``dtype="fp8"`` writes version 6, with ``rescore=True`` version 7, whose rescore block is the stored bf16 rows
    gathered into id order. ``ivf=nlist`` (a plain ``src``, version 1 or 2) builds the lists over the stored rows
    with :func:`ivf_kmeans` / :func:`ivf_layout` (``nprobe``, ``ivf_seed``, ``ivf_iters`` as in
    :func:`write_index`): version 5 for ``dtype="bf16"``, 6 or 7 for fp8. A deleted row keeps its id, is assigned to
    a list and stays dead. ``ivf_backend="gpu"``: the lists come from :func:`cluster_rows` on ``device``.
    ``dtype="pq"`` (a plain ``src``, ``pq_m`` code bytes per row): the stored rows are trained on (:func:`pq_train` with
    ``pq_seed`` / ``pq_iters``, unless ``pq_codebook`` is given) and encoded as they stand, which gives the bytes
    ``write_index(dtype="pq")`` stores for the same vectors and codebook: version 10, with ``rescore=True`` 11.
    ``pq_backend`` as in :func:`write_index`."""
    _check_ivf_backend(ivf_backend, ivf)
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {tuple(DTYPES)}, got {dtype!r}")
    _check_pq_backend(pq_backend, "pq_backend")
    if dtype != "pq" and (pq_m is not None or pq_codebook is not None or pq_seed != 0 or pq_iters != 10 or pq_backend != "cpu"):
        raise ValueError(f"pq_m, pq_codebook, pq_seed, pq_iters and pq_backend go with dtype='pq', got dtype={dtype!r}")
    if dtype == "pq" and ivf is not None:
        raise ValueError(f"ivf={ivf!r} with dtype='pq': IVF lists over pq8 rows are not built")
    if dtype == "pq" and pq_m is None:
        raise ValueError("dtype='pq' needs pq_m, the code bytes per row (a multiple of 16 in 16..96 that divides dim)")
    if rescore and dtype not in ("fp8", "bin", "pq"):
        raise ValueError(f"rescore rows go with an fp8 index: a {dtype} index already holds its rows in bf16")
    if dtype == "bin" and ivf is not None:
        raise ValueError(f"ivf={ivf!r} with dtype='bin': IVF lists over binary rows are not built")
    hdr = read_header(src)
    if dtype == "pq":
        if hdr["dtype"] != "bf16" or "ivf" in hdr:
            raise ValueError(f"dtype='pq': {src} holds {hdr['dtype']} rows{' in IVF lists' if 'ivf' in hdr else ''}, and a pq8 "
                             f"index is converted from a plain bf16 index")
        check_pq_shape(hdr["dim"], pq_m)
    if dtype == "bin" and hdr["dtype"] != "bf16":
        raise ValueError(f"dtype='bin': {src} holds {hdr['dtype']} rows, and a binary index is converted from a plain bf16 "
                         f"index (its sign bits are the vectors' own)")
    if hdr["dtype"] != "bf16":
        raise ValueError(f"{src}: only a bf16 index can be converted, this one holds {hdr['dtype']}")
    if ivf is None and (nprobe is not None or ivf_seed != 0 or ivf_iters != 10):
        raise ValueError(f"nprobe={nprobe!r}, ivf_seed={ivf_seed!r} and ivf_iters={ivf_iters!r} go with ivf=nlist")
    if ivf is not None and "ivf" in hdr:
        raise ValueError(f"ivf={ivf!r}: {src} is an IVF index already (nlist {hdr['ivf']['nlist']}); its lists are kept")
    if dtype == "fp8" and hdr["dim"] % 16:
        raise ValueError(f"dim of an fp8 index must be a multiple of 16 in 16..2048, got {hdr['dim']}")
    if dtype == "bin":
        if "ivf" in hdr:
            raise ValueError(f"dtype='bin': {src} is an IVF index (nlist {hdr['ivf']['nlist']}), and IVF lists over binary "
                             f"rows are not built")
        if hdr["dim"] % 128 or hdr["dim"] < 128:
            raise ValueError(f"dim of a binary index must be a multiple of 128 in 128..2048, got {hdr['dim']}")
    bits, scales = read_rows(src), None
    out = {k: hdr[k] for k in ("dim", "count") if k in hdr}
    out.update(dtype=DTYPES[dtype], metric=hdr["metric"], model=hdr.get("model", ""), embed=hdr.get("embed"))
    if hdr.get("labels") is not None:
        out["labels"] = hdr["labels"]
    v2 = "tags_off" in hdr
    if ivf is not None or "ivf" in hdr:
        if "ivf" in hdr:  # the stored order, the tables and the centroids as they are
            lay = {k: v for k, v in read_ivf(src).items() if k not in ("pos", "list_of")}
            tags, live = read_tags(src), read_live(src)
            real = lay["rowid"] >= 0
        else:
            n = hdr["count"]
            nlist, nprobe = _check_ivf_args(n, ivf, nprobe, ivf_seed, ivf_iters)
            cbits, assign = _ivf_lists(bits, nlist, hdr["metric"], int(ivf_seed), int(ivf_iters), ivf_backend, device, dst)
            lay = ivf_layout(assign, nlist)
            real = lay["rowid"] >= 0
            ids = lay["rowid"][real]
            rows, bits = bits, np.zeros((real.size, hdr["dim"]), np.uint16)
            bits[real] = rows[ids]
            tags, live = np.zeros(real.size, np.uint32), np.zeros(real.size, bool)
            tags[real] = read_tags(src)[ids] if v2 else 0
            live[real] = read_live(src)[ids] if v2 else True
            lay.update(centroids=cbits, nlist=nlist, nprobe=nprobe, seed=int(ivf_seed), iters=int(ivf_iters))
        rrows = None
        if rescore:  # the stored rows gathered into id order: what a plain bf16 index of the vectors holds
            rrows = np.empty((hdr["count"], hdr["dim"]), np.uint16)
            rrows[lay["rowid"][real]] = bits[real]
        if dtype == "fp8":  # padding rows: code 0, scale 1 (and dead)
            codes, scales = np.zeros(bits.shape, np.uint8), np.ones(bits.shape[0], np.float32)
            codes[real], scales[real] = quantize_rows(bf16_to_f32(bits[real]))
            bits = codes
        return _write_file(dst, out, bits, tags, live, scales=scales, rescore=rrows, ivf=lay)
    rrows = bits if rescore else None
    if dtype == "fp8":
        bits, scales = quantize_rows(bf16_to_f32(bits))
    if dtype == "bin":  # the sign bits of the stored rows: what binarising the fp32 vectors gives
        bits = binarize_bf16(bits)
    codebook = None
    if dtype == "pq":  # trained on and encoded from the stored rows as they stand (prepare_rows_pq rounds to bf16 first)
        rows32 = bf16_to_f32(bits)
        codebook = pq_train(rows32, pq_m, seed=pq_seed, iters=pq_iters, backend=pq_backend, device=device) \
            if pq_codebook is None else check_codebook(pq_codebook, hdr["dim"], pq_m)
        bits = pq_encode(rows32, codebook, backend=pq_backend, device=device)
    return _write_file(dst, out, bits, read_tags(src) if v2 else None, read_live(src) if v2 else None,
                       hdr.get("capacity"), scales=scales, rescore=rrows, pq=codebook)
