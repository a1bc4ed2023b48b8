"""The cases behind tests/golden/batch_bits.npz: the three MFMA batch scans (kinds MSCAN, XSCAN and PQXSCAN), each
followed by MERGEN, whose merged scores and ids are recorded bit for bit (scripts/batch_bits_record.py) and compared
by tests/test_batch_bits_gpu.py.

Inputs come from the closed-form integer recipe of search_bits_cases (``mix``: numpy integer arithmetic only, no RNG
library), so the fixture stores outputs only. Rows and table entries are bf16 bit patterns with mixed signs over six
binades (2^-3 .. 2^2) and 7-bit mantissas, queries fp32 bit patterns with full 23-bit mantissas: every fp32 partial
sum inside the MFMA chain is inexact, and a changed order of the additions changes bits.

Every case has N = 300 rows (two tiles, the second ragged at 44 rows) and the live bitmap LIVE: one all-dead group
of 16 (rows 16..31), a mixed group (rows 40 and 45 dead in 32..47) and a wave whose 64 rows are all dead (64..127).
Dead row 40 holds 0x7FC0 (a NaN) in every column; for PQXSCAN it holds code 255 in every byte, the table's entry 255
is 0x7FC0 throughout and no live row uses that code."""
import numpy as np

from hipzap import search as S

from search_bits_cases import mix, save_fixture  # noqa: F401  (save_fixture is re-exported)
from search_filter_cases import subset_ambiguous  # noqa: F401  (re-exported)

N = 300
NAN_ROW, DEAD_QID, OUT_QID = 40, 45, N + 7  # MSCAN: one qid names the deleted row 45, one lies outside [0, N)
LIVE = np.ones(N, bool)
LIVE[16:32] = False
LIVE[[NAN_ROW, DEAD_QID]] = False
LIVE[64:128] = False

# (name, kind, D, M or skip_self, Q, k, salt). Q = 17: one query past a group of 16. Q = 65: a second query block of one
# query, three of whose query groups are skipped. k = 10: the radix cut; k = 128: the k > 64 path (Q = 3 keeps the file
# small). MSCAN: D / 32 = 1 .. 5, every tail of the four-step loop. PQXSCAN: (D, M) with 4, 8, 8 and 12 k-steps and
# one, one, two and three 16-byte code chunks per row; (256, 16) has two table chunks per sub-space. The salts are the
# smallest for which every query's fp64 top k is forced under twice the error bound (found on the host, asserted by the
# CPU test for the k = 10 cases; at k = 128 of 218 live rows some neighbours are always closer than that).
CASES = [
    ("mscan_d32_self", "mscan", 32, 0, 17, 10, 0), ("mscan_d64", "mscan", 64, 1, 17, 10, 1),
    ("mscan_d96_self", "mscan", 96, 0, 17, 10, 0), ("mscan_d128", "mscan", 128, 1, 17, 10, 0),
    ("mscan_d160_self", "mscan", 160, 0, 17, 10, 0), ("mscan_d64_q65", "mscan", 64, 1, 65, 10, 2),
    ("mscan_d32_k128", "mscan", 32, 1, 3, 128, 0),
    ("xscan_d32", "xscan", 32, 0, 17, 10, 0), ("xscan_d64", "xscan", 64, 0, 17, 10, 0), ("xscan_d96", "xscan", 96, 0, 17, 10, 1),
    ("xscan_d32_q65", "xscan", 32, 0, 65, 10, 0), ("xscan_d64_k128", "xscan", 64, 0, 3, 128, 0),
    ("pqx_d128_m16", "pqx", 128, 16, 17, 10, 0), ("pqx_d256_m16", "pqx", 256, 16, 17, 10, 8),
    ("pqx_d256_m32", "pqx", 256, 32, 17, 10, 4), ("pqx_d384_m48", "pqx", 384, 48, 17, 10, 652),
    ("pqx_d128_m16_q65", "pqx", 128, 16, 65, 10, 7), ("pqx_d128_m16_k128", "pqx", 128, 16, 3, 128, 0),
]
NAMES = [c[0] for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


def _bf16(x):
    """Hash words -> bf16 bits: sign, one of six binades 2^-3 .. 2^2, seven mantissa bits."""
    return (((x & np.uint64(1)) << np.uint64(15)) | ((((x >> np.uint64(1)) % np.uint64(6)) + np.uint64(124)) << np.uint64(7)) |
            ((x >> np.uint64(8)) & np.uint64(0x7F))).astype(np.uint16)


def _f32(y):
    """Hash words -> fp32: sign, one of four binades 2^-2 .. 2^1, 23 mantissa bits."""
    return (((y & np.uint64(1)) << np.uint64(31)) | ((((y >> np.uint64(1)) % np.uint64(4)) + np.uint64(125)) << np.uint64(23)) |
            ((y >> np.uint64(5)) & np.uint64(0x7FFFFF))).astype(np.uint32).view(np.float32)


def inputs(name):
    """-> dict: bits (the bf16 rows the scan multiplies, uint16 [N, D]; for pqx the decoded rows), live, and per kind
    qid (int32 [Q]) and skip_self / q (fp32 [Q, D]) / q, codes (uint8 [N, M]) and cb8 (uint16 [D / 8, 256, 8])."""
    _, kind, D, arg, Q, k, salt = case(name)
    key = 16 * D + 8192 * salt + {"mscan": 1, "xscan": 2, "pqx": 3}[kind]
    out = {"live": LIVE}
    if kind == "pqx":
        M = arg
        cb8 = _bf16(mix(np.arange(D // 8 * 256)[:, None], np.arange(8)[None, :], key)).reshape(D // 8, 256, 8)
        cb8[:, 255, :] = 0x7FC0
        codes = (mix(np.arange(N)[:, None], np.arange(M)[None, :], key + 4) % np.uint64(255)).astype(np.uint8)  # 0 .. 254
        codes[NAN_ROW] = 255
        out.update(codes=codes, cb8=cb8, bits=S.pq_decode_bf16(codes, cb8))
    else:
        bits = _bf16(mix(np.arange(N)[:, None], np.arange(D)[None, :], key))
        bits[NAN_ROW] = 0x7FC0
        out["bits"] = bits
    if kind == "mscan":
        live_rows = np.flatnonzero(LIVE)
        qid = live_rows[(mix(np.arange(Q), 0, key + 5) % np.uint64(live_rows.size)).astype(np.int64)].astype(np.int32)
        qid[0] = 299  # the last row of the ragged tile
        if Q >= 17:
            qid[5], qid[11] = DEAD_QID, OUT_QID
        out.update(qid=qid, skip_self=arg)
    else:
        q = _f32(mix(np.arange(Q)[:, None], np.arange(D)[None, :], key + 6))
        if Q >= 17:  # components below 2^-102: split_term flushes the m and l terms (and h of the subnormal)
            q[3, 1], q[3, D - 2], q[3, 7] = np.float32(1.5 * 2.0 ** -110), np.float32(-1.25 * 2.0 ** -120), np.float32(2.0 ** -140)
        out["q"] = q
    return out


def oracle(name, inp):
    """-> (fp64 scores [Q, N] of the effective queries against the rows, the error bounds [Q, N], allow bool [Q, N]).
    The bound is hipzap.h's: beta(n) * sum |terms| |row| with n = 3 D additions for the split query, D for a bf16 one."""
    _, kind, D, arg, Q, k, salt = case(name)
    rows = S.bf16_to_f32(inp["bits"]).astype(np.float64)
    rows[~LIVE] = 0.0  # a dead row never passes; keep its NaN out of the products
    allow = np.repeat(LIVE[None, :], Q, axis=0)
    if kind == "mscan":
        qid = inp["qid"]
        real = (qid >= 0) & (qid < N)
        eff = np.where(real[:, None], S.bf16_to_f32(inp["bits"][np.where(real, qid, 0)]).astype(np.float64), 0.0)
        eff[~np.isfinite(eff)] = 0.0
        mag, n = np.abs(eff), D
        allow &= real[:, None]
        if arg:
            allow[np.flatnonzero(real), qid[real]] = False
    else:
        h, m, l = (t.astype(np.float64) for t in S.split3(inp["q"]))
        eff, mag, n = h + m + l, np.abs(h) + np.abs(m) + np.abs(l), 3 * D
    u = n * 2.0 ** -23
    return eff @ rows.T, u / (1 - u) * (mag @ np.abs(rows).T), allow


def ref_ids(name, inp):
    s, _, allow = oracle(name, inp)
    k = case(name)[5]
    ids = np.full((s.shape[0], k), -1, np.int32)
    for qi in range(s.shape[0]):
        rows = np.flatnonzero(allow[qi])
        order = rows[np.lexsort((rows, -s[qi, rows]))][:k]  # higher score first, then the lower id
        ids[qi, :order.size] = order
    return ids


def run_case(name):
    """One scan + MERGEN launch pair on the GPU -> (score bits uint32 [Q, k], ids int32 [Q, k])."""
    _, kind, D, arg, Q, k, salt = case(name)
    inp = inputs(name)
    if kind == "mscan":
        from test_search_neighbors_gpu import launch
        rs, rm, sc, ids = launch(inp["bits"], inp["qid"], k, LIVE, arg)
    elif kind == "xscan":
        from test_search_batch_gpu import launch
        rs, rm, sc, ids = launch(inp["bits"], inp["q"], k, LIVE)
    else:
        from test_search_pqbatch_gpu import launch
        rs, rm, sc, ids = launch(inp["codes"], inp["cb8"], inp["q"], k, LIVE)
    assert (rs, rm) == (0, 0), (name, rs, rm)
    return np.ascontiguousarray(sc, np.float32).view(np.uint32), np.ascontiguousarray(ids, np.int32)
