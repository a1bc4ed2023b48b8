"""The cases of the fp8 IVF tests, shared by tests/test_search_ivf_fp8_cpu.py (which asserts on the
host that every index-level query is forced), tests/test_search_ivf_fp8_gpu.py (the quantised list-scan kernel
through its launcher) and tests/test_search_ivf_fp8_index_gpu.py (the GPU index over version-6 and version-7 files).

Bounds: stage one is the fp8 scan's (``search_fp8_cases.oracle_q``: gamma(D + 1) * |scale| * sum |q c|), the coarse
stage and stage two are the bf16 scan's (``oracle``: gamma(D) * sum |q r|)."""
import numpy as np

from hipzap import search as S

import search_fp8_cases as P
import search_ivf_cases as V
import search_rescore_cases as R
from search_ivf_cases import (DUP, IX_D, IX_LISTS, IX_N, IX_Q, LIST_OFF, LIST_TILES, N_EXT, NLIST, NTILE, T,  # noqa: F401
                              ambiguous, clustered_data, index_tags, kernel_probes, oracle, probe_tiles)

MAX_K = R.MAX_K
NAN_CODE = 0x7F  # e4m3fn NaN: what the padding rows hold at kernel level, with NaN scales

# (name, D, Q, k, nprobe, user filter): every D of {16, 528, 1024, 1040, 2048} (NC 1 and 2, the NC boundary, lanes
# past a row's end), Q of {1, 3, 16}, k of {1, 10, 128} and nprobe of {1, 2, 5} appears
KCASES = [
    ("d16_q1_k1_p1", 16, 1, 1, 1, False),
    ("d16_q16_k10_p2", 16, 16, 10, 2, False),
    ("d528_q3_k128_p5", 528, 3, 128, 5, False),
    ("d528_q16_k1_p2", 528, 16, 1, 2, True),
    ("d1024_q3_k10_p1", 1024, 3, 10, 1, True),
    ("d1024_q1_k128_p2", 1024, 1, 128, 2, False),
    ("d1040_q16_k10_p5", 1040, 16, 10, 5, False),
    ("d2048_q3_k128_p1", 2048, 3, 128, 1, True),
    ("d2048_q16_k10_p2", 2048, 16, 10, 2, False),
]
KNAMES = [c[0] for c in KCASES]


def kernel_layout(D, Q, seed=31):
    """``search_ivf_cases.kernel_layout`` through the quantiser: ``codes`` uint8 [7 T, D] and ``scales`` fp32 [7 T]
    in stored order (a real row: ``quantize_rows`` of its bf16 values; padding: NaN codes and NaN scales), plus the
    layout's ``rowid``, ``live``, ``tags``, ``list_of`` and ``q``."""
    lay = V.kernel_layout(D, Q, seed)
    live = lay["live"]
    codes = np.full(lay["bits"].shape, NAN_CODE, np.uint8)
    scales = np.full(live.size, np.nan, np.float32)
    codes[live], scales[live] = S.quantize_rows(S.bf16_to_f32(lay["bits"][live]))
    return dict(lay, codes=codes, scales=scales)


# ------------------------------------------------------------------------------ the index-level scenario
COVER_FILTER = (0xFFFFFFFF, 3)  # index_tags() == 3: at most 44 rows per list pass, so R = 128 covers any two lists


def write_files(tmp):
    """The IX scenario of ``search_ivf_cases`` in every form -> dict of paths: ``v5`` (the bf16 IVF file), ``v6`` and
    ``v7`` (converted from it), ``plain`` (bf16), ``p3`` and ``p4`` (the plain fp8 and two-stage conversions)."""
    v, _ = clustered_data()
    f = {k: str(tmp / f"{k}.hzidx") for k in ("plain", "v5", "v6", "v7", "p3", "p4")}
    S.write_index(f["plain"], v, "cosine", tags=index_tags())
    S.write_index(f["v5"], v, "cosine", tags=index_tags(), ivf=IX_LISTS, nprobe=2)  # lists of 93, 62, 91, 45, 219, 90 rows
    S.convert_index(f["v5"], f["v6"], "fp8")
    S.convert_index(f["v5"], f["v7"], "fp8", rescore=True)
    S.convert_index(f["plain"], f["p3"], "fp8")
    S.convert_index(f["plain"], f["p4"], "fp8", rescore=True)
    return f


def probes_forced(ref, q, nprobe):
    """-> (bool [Q]: the gap between neighbouring centroid scores up to the nprobe-th and the next is above twice
    their bounds, bool [Q, N]: the rows of the lists the oracle probes)."""
    nlist = ref.ivf["nlist"]
    ok, near = np.ones(q.shape[0], bool), np.ones((q.shape[0], ref.count), bool)
    if nprobe >= nlist:
        return ok, near
    cs, cb, _, _ = oracle(ref._cent, q, nprobe)
    for qi in range(q.shape[0]):
        order = np.argsort(-cs[qi], kind="stable")
        srt, bs = cs[qi][order], cb[qi][order]
        ok[qi] = not (srt[:-1] - srt[1:] <= 2 * np.maximum(bs[:-1], bs[1:]))[:nprobe].any()
        near[qi] = np.isin(ref.ivf["list_of"], order[:nprobe])
    return ok, near


def forced(ref, q, k, nprobe, refine=0, allow=None):
    """The host criterion that the answer of ``ref`` (a RefIndex of a version-6 or version-7 file) is determined
    -> bool [Q]. The probes are forced (``probes_forced``); over the passing rows of the probed lists, with
    ``refine`` = 0 the fp8 top k is unambiguous under the fp8 bound, and with ``refine`` = R (a) every member of
    the bf16 top k stands inside the fp8 top R by more than twice the largest fp8 bound and (b) the bf16 top k is
    unambiguous under the bf16 bound (``search_rescore_cases``)."""
    q = np.asarray(q, np.float32)
    out, near = probes_forced(ref, q, nprobe)
    s8, b8 = P.oracle_q(ref._bits, ref.scales, q)
    if refine:
        s16, b16, _, _ = oracle(ref._rrows, q, k)
    for qi in range(q.shape[0]):
        rows = np.flatnonzero(near[qi] & ref._live & (True if allow is None else allow))
        if not rows.size:
            continue
        if not refine:
            out[qi] &= not ambiguous(s8[qi:qi + 1, rows], b8[qi:qi + 1, rows], k)
            continue
        out[qi] &= not ambiguous(s16[qi:qi + 1, rows], b16[qi:qi + 1, rows], k)
        if rows.size > refine:
            order8 = rows[np.argsort(-s8[qi, rows], kind="stable")]
            top16 = rows[np.argsort(-s16[qi, rows], kind="stable")[:k]]
            out[qi] &= bool(np.all(s8[qi, top16] - s8[qi, order8[refine]] > 2 * b8[qi, rows].max()))
    return out
