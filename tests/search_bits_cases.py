"""The cases behind tests/golden/search_bits.npz: one launch per scan instantiation (and each format's largest D)
whose scores and ids are recorded bit for bit (scripts/search_bits_record.py) and compared by
tests/test_search_bits_gpu.py.

Inputs come from a closed-form integer recipe (numpy integer arithmetic only, no RNG library), so the fixture
stores outputs only and cannot drift with a numpy version. Rows are bf16 bit patterns or e4m3 codes with mixed
signs and exponents over six binades (2^-3 .. 2^2), queries are fp32 bit patterns with full 23-bit mantissas, so
every fp32 partial sum is inexact and a changed summation order changes bits. No NaN or inf pattern occurs (the
exponent fields stay far below all-ones, which also excludes the e4m3 NaN codes 0x7F / 0xFF). Scales have a
nonzero mantissa: no power of two."""
import io
import zipfile

import numpy as np

from hipzap import search as S

from search_filter_cases import T, gamma, subset_ambiguous  # noqa: F401  (re-exported)

N, Q, K = T + 5, 3, 10  # two tiles, the second partial
# (name, kind, D, salt): the smallest D of every NC and the largest D, per kind. The salts are the smallest for which
# the fp64 top-k is forced under the fp32 bound (found on the host, asserted by the CPU test).
SALTS = {"scan": {8: 0, 520: 0, 1032: 1, 1544: 0, 2048: 1}, "fscan": {8: 0, 520: 0, 1032: 0, 1544: 10, 2048: 1},
         "qscan": {16: 0, 1040: 0, 2048: 5}}
CASES = [(f"{kind}_d{d}", kind, d, salt) for kind, ds in SALTS.items() for d, salt in ds.items()]
NAMES = [c[0] for c in CASES]
FILT = np.array([[0, 0], [3, 1], [4, 4]], np.uint32)  # per query {mask, value}: all rows, tag % 4 == 1, tag bit 2 set


def mix(i, j, salt):
    """A 32-bit integer hash of (i, j, salt), elementwise, in uint64 arithmetic."""
    x = (np.asarray(i, np.uint64) * np.uint64(2654435761) + np.asarray(j, np.uint64) * np.uint64(40503) +
         np.uint64(salt) * np.uint64(2246822519) + np.uint64(374761393)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def _grid(n, d, salt):
    return mix(np.arange(n)[:, None], np.arange(d)[None, :], salt)


def inputs(kind, D, salt=0):
    """-> dict: rows (bf16 bits uint16 or e4m3 codes uint8 [N, D]), rows32 (the rows as fp32), scales (fp32 [N] or
    None), q (fp32 [Q, D]), live (bool [N]), tags (uint32 [N]), allow (bool [Q, N]: which (q, r) pass)."""
    x = _grid(N, D, D + 4096 * salt)
    sign, binade = x & np.uint64(1), (x >> np.uint64(1)) % np.uint64(6)
    if kind == "qscan":
        rows = ((sign << np.uint64(7)) | ((binade + np.uint64(4)) << np.uint64(3)) | ((x >> np.uint64(8)) & np.uint64(7))).astype(np.uint8)
        rows32 = S.e4m3_to_f32(rows)
        r = np.arange(N, dtype=np.uint64)
        scales = ((((r % np.uint64(5)) + np.uint64(120)) << np.uint64(23)) |
                  (((r * np.uint64(7919) + np.uint64(12345)) % np.uint64(0x7FFFFF)) | np.uint64(1))).astype(np.uint32).view(np.float32)
    else:
        rows = ((sign << np.uint64(15)) | ((binade + np.uint64(124)) << np.uint64(7)) | ((x >> np.uint64(8)) & np.uint64(0x7F))).astype(np.uint16)
        rows32, scales = S.bf16_to_f32(rows), None
    y = _grid(Q, D, D + 4096 * salt + 1)
    q = (((y & np.uint64(1)) << np.uint64(31)) | ((((y >> np.uint64(1)) % np.uint64(4)) + np.uint64(125)) << np.uint64(23)) |
         ((y >> np.uint64(5)) & np.uint64(0x7FFFFF))).astype(np.uint32).view(np.float32)
    z = mix(np.arange(N), 0, D + 4096 * salt + 2)
    live, tags = np.ones(N, bool), (z % np.uint64(8)).astype(np.uint32)
    allow = np.ones((Q, N), bool)
    if kind != "scan":
        live = (z >> np.uint64(8)) % np.uint64(5) != 0
        live[8:12] = False  # one all-dead group of four rows: the kernel skips it whole
        allow = live[None, :] & ((tags[None, :] & FILT[:, :1]) == FILT[:, 1:])
    return {"rows": rows, "rows32": rows32, "scales": scales, "q": q, "live": live, "tags": tags, "allow": allow}


def oracle(inp):
    """fp64 scores [Q, N] and the fp32 error bounds [Q, N] of the existing suites (gamma(D + 1) with a scale)."""
    c, q = inp["rows32"].astype(np.float64), inp["q"].astype(np.float64)
    D = c.shape[1]
    s, b = q @ c.T, np.abs(q) @ np.abs(c).T
    if inp["scales"] is None:
        return s, gamma(D) * b
    sc = inp["scales"].astype(np.float64)
    return s * sc, gamma(D + 1) * b * np.abs(sc)


def ref_ids(inp):
    return S.search_ref(inp["rows32"], inp["q"], K, inp["allow"], scales=inp["scales"])[1]


def run_case(name):
    """One scan + merge launch pair on the GPU -> (score bits uint32 [Q, K], ids int32 [Q, K])."""
    _, kind, D, salt = CASES[NAMES.index(name)]
    inp = inputs(kind, D, salt)
    if kind == "scan":
        from test_search_gpu import launch
        rs, rm, sc, ids = launch(inp["rows"], inp["q"], K)
    elif kind == "fscan":
        from test_search_filter_gpu import launch
        rs, rm, sc, ids = launch(inp["rows"], inp["q"], K, inp["live"], inp["tags"], FILT)
    else:
        from test_search_fp8_gpu import launch
        rs, rm, sc, ids = launch(inp["rows"], inp["scales"], inp["q"], K, inp["live"], inp["tags"], FILT)
    assert (rs, rm) == (0, 0), (name, rs, rm)
    return np.ascontiguousarray(sc, np.float32).view(np.uint32), np.ascontiguousarray(ids, np.int32)


def save_fixture(path, arrays):
    """An uncompressed .npz with fixed member times: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), version=(1, 0))
            z.writestr(zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue())
