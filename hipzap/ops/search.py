"""Vector search kernels (csrc/search.hip): exact top-k by inner product over a bf16 corpus.

``HzSearchParams`` is the parameter block of both kinds: ``HZ_K_SEARCH_SCAN`` (one workgroup per tile
of ``tile_rows()`` corpus rows, all queries of the launch resident in LDS, the tile's best ``k`` keys per
query into ``cand``) and ``HZ_K_SEARCH_MERGE`` (one workgroup per query, ``ntile x k`` keys -> the final
``k``). ``HZ_K_SEARCH_FSCAN`` (``FilterScanParams``: the same block plus a live bitmap, per-row tags and
per-query ``{mask, value}`` filters) is the scan over the rows that pass. ``HZ_K_SEARCH_QSCAN``
(``QuantScanParams``: that block plus one fp32 scale per row) is the filtered scan over rows of OCP e4m3fn bytes.
``HZ_K_SEARCH_BSCAN`` (``BinScanParams``: the filtered block over uint32 sign-bit rows, ``ldc`` in words) scores
``D - 2 popcount(query bits xor row bits)``, the queries binarised in the kernel.
``HZ_K_SEARCH_RESCORE`` (``RescoreParams``) is the second stage of a two-stage search: one workgroup per query
re-scores the ``R`` bf16 rows that a merge's ``out_id`` names and writes the best ``k`` of them.
``HZ_K_SEARCH_LSCAN`` (``ListScanParams``) is the filtered scan over an IVF index's lists: workgroup (j, q) scans
the j-th tile of the lists that ``probes[q]`` names; ``HZ_K_SEARCH_QLSCAN`` (``QuantListScanParams``: that block plus
one fp32 scale per stored row) is the list scan over rows of e4m3fn bytes.
``HZ_K_SEARCH_MSCAN`` (``SelfScanParams``) scores rows of the corpus, named by ``qid``, against every tile with the
bf16 MFMA, ``SELF_QB`` queries a workgroup; ``HZ_K_SEARCH_MERGEN`` is the merge for any number of queries over the
same block.
``HZ_K_SEARCH_XSCAN`` (``BatchScanParams``: that block with device fp32 ``queries`` where ``qid`` is) is the self scan
over external queries, each split into three bf16 terms; ``HZ_K_SEARCH_MERGEN`` takes its block as it stands and
``HZ_K_SEARCH_RESCOREN`` is the rescore (``RescoreParams``) for any number of queries.
``HZ_K_SEARCH_ASSIGN`` (``AssignParams``) writes the nearest of ``C`` bf16 centroids for every row of a tile with the
same MFMA, ``HZ_K_SEARCH_CMEAN`` (``CmeanParams``) the means of the clusters ``order`` / ``seg_off`` describe.
``HZ_K_SEARCH_PQLUT`` (``PqLutParams``) writes each query's table of inner products with the 256 sub-centroids of every
sub-space of a product quantiser; ``HZ_K_SEARCH_PQSCAN`` (``PqScanParams``: the filtered block over uint8 code rows,
``ldc`` in bytes, plus the table) adds M table entries per row, one query's table resident in LDS per workgroup.
``HZ_K_SEARCH_PQASSIGN`` (``PqAssignParams``) writes, for every bf16 row and sub-space, the nearest of the 256
sub-centroids under squared L2 in plain fp32 operations (:func:`hipzap.search.pq_assign_f32` is its bits in numpy);
``pq_encode_rows`` is the batch job over host rows built on it (``hz_pq_encode``).
torch-free: indexes (:mod:`hipzap.search`) are served without it."""
from __future__ import annotations

import ctypes as C

from .. import _native as N

MAX_Q, MAX_K = 16, 128  # HZ_SEARCH_MAX_Q, HZ_SEARCH_MAX_K (csrc/hipzap.h)
SELF_QB = 64                     # HZ_SEARCH_SELF_QB: queries per workgroup of the self scan
SELF_MAX_Q = 65535 * SELF_QB     # HZ_SEARCH_SELF_MAX_Q: the self scan's and its merge's limit on Q
INDEX_SELF_MAX_Q = 1024          # HZ_INDEX_SELF_MAX_Q: ids per hz_index_neighbors call
ASSIGN_CB = 64                   # HZ_SEARCH_ASSIGN_CB: centroids per block of the assign kernel
ASSIGN_MAX_C = 65536             # HZ_SEARCH_ASSIGN_MAX_C: the most centroids (hipzap.search.IVF_MAX_LISTS)
PQ_MAX_M, PQ_MAX_DSUB, PQ_KSUB = 96, 64, 256  # HZ_SEARCH_PQ_MAX_M, HZ_SEARCH_PQ_MAX_DSUB; sub-centroids per sub-space


@N.params_of("HZ_K_SEARCH_MERGE")
@N.params_of("HZ_K_SEARCH_SCAN")
class SearchParams(C.Structure):
    _fields_ = [("corpus", C.c_void_p), ("queries", C.c_void_p), ("cand", C.c_void_p), ("out_score", C.c_void_p),
                ("out_id", C.c_void_p), ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int),
                ("ldc", C.c_int), ("ntile", C.c_int), ("cand_bytes", C.c_uint64)]


_FILTER_FIELDS = [("live", C.c_void_p), ("tags", C.c_void_p), ("filt", C.c_void_p), ("live_bytes", C.c_uint64)]


@N.params_of("HZ_K_SEARCH_FSCAN")
class FilterScanParams(C.Structure):
    """HzSearchFilterParams: the fields of ``SearchParams``, then the filter's."""
    _fields_ = SearchParams._fields_ + _FILTER_FIELDS

    def scan_params(self) -> SearchParams:
        """The leading ``SearchParams`` of this block (what the merge takes)."""
        return SearchParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_QSCAN")
class QuantScanParams(C.Structure):
    """HzSearchQuantParams: the fields of ``FilterScanParams`` (``corpus``: uint8 rows, ``ldc`` in bytes), then
    ``scales`` (fp32 [N])."""
    _fields_ = FilterScanParams._fields_ + [("scales", C.c_void_p)]

    def scan_params(self) -> SearchParams:
        return SearchParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_BSCAN")
class BinScanParams(C.Structure):
    """HzSearchBinParams: the fields of ``FilterScanParams`` (``corpus``: uint32 sign-bit rows [N][ldc], ``ldc`` in
    words; ``live`` is required)."""
    _fields_ = list(FilterScanParams._fields_)

    def scan_params(self) -> SearchParams:
        """The merge's block: it reads no row, but checks a bf16 pitch, so ``ldc`` = D there."""
        sp = SearchParams.from_buffer_copy(self)
        sp.ldc = sp.D
        return sp


@N.params_of("HZ_K_SEARCH_PQLUT")
class PqLutParams(C.Structure):
    """HzSearchPqLutParams: ``queries`` fp32 [Q][D], ``codebook`` fp32 [M][256][D / M], ``lut`` fp32 [Q][M][256] out."""
    _fields_ = [("queries", C.c_void_p), ("codebook", C.c_void_p), ("lut", C.c_void_p), ("lut_bytes", C.c_uint64),
                ("D", C.c_int), ("M", C.c_int), ("Q", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_SEARCH_PQSCAN")
class PqScanParams(C.Structure):
    """HzSearchPqParams: the fields of ``FilterScanParams`` (``corpus``: uint8 code rows [N][ldc], ``ldc`` in bytes;
    ``live`` is required), then ``lut`` (the table kind's output), ``lut_bytes``, ``M`` and ``span`` (0: the
    launcher's choice)."""
    _fields_ = FilterScanParams._fields_ + [("lut", C.c_void_p), ("lut_bytes", C.c_uint64), ("M", C.c_int),
                                            ("span", C.c_int)]

    def scan_params(self) -> SearchParams:
        """The merge's block: it reads no row, but checks a bf16 pitch, so ``ldc`` = D there."""
        sp = SearchParams.from_buffer_copy(self)
        sp.ldc = sp.D
        return sp


@N.params_of("HZ_K_SEARCH_PQASSIGN")
class PqAssignParams(C.Structure):
    """HzSearchPqAssignParams: ``rows`` bf16 [N][ldr], ``codebook`` fp32 [M][256][D / M], ``codes`` uint8 [N][ldc] out
    (``ldc`` in bytes), ``dist`` fp32 [N][M] out or null with ``dist_bytes``."""
    _fields_ = [("rows", C.c_void_p), ("codebook", C.c_void_p), ("codes", C.c_void_p), ("dist", C.c_void_p),
                ("dist_bytes", C.c_uint64), ("N", C.c_longlong), ("D", C.c_int), ("M", C.c_int),
                ("ldr", C.c_longlong), ("ldc", C.c_longlong)]


@N.params_of("HZ_K_SEARCH_RESCOREN")
@N.params_of("HZ_K_SEARCH_RESCORE")
class RescoreParams(C.Structure):
    """HzSearchRescoreParams: ``rows`` bf16 [N][ldc] (device or mapped pinned host memory), ``queries`` fp32
    [Q][D], ``in_id`` int32 [Q][R] (-1: an empty slot), the outputs [Q][k]."""
    _fields_ = [("rows", C.c_void_p), ("queries", C.c_void_p), ("in_id", C.c_void_p), ("out_score", C.c_void_p),
                ("out_id", C.c_void_p), ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("R", C.c_int),
                ("k", C.c_int), ("ldc", C.c_int)]


@N.params_of("HZ_K_SEARCH_LSCAN")
class ListScanParams(C.Structure):
    """HzSearchListParams: the fields of ``FilterScanParams`` (``N`` stored rows, whole tiles; ``cand`` holds
    [P][Q][k] keys), then ``probes`` (device int32 [Q][nprobe], or 0: every list), ``list_off`` (int32 [nlist + 1]),
    ``list_tiles`` (int32 [N / tile_rows()]), ``rowid`` (int32 [N]) and ``nlist``, ``nprobe``, ``P``."""
    _fields_ = FilterScanParams._fields_ + [("probes", C.c_void_p), ("list_off", C.c_void_p), ("list_tiles", C.c_void_p),
                                            ("rowid", C.c_void_p), ("nlist", C.c_int), ("nprobe", C.c_int),
                                            ("P", C.c_int), ("pad_", C.c_int)]

    def merge_params(self) -> SearchParams:
        """The merge's block for this scan's candidates: ``ntile`` = P, so N = P * 256."""
        sp = SearchParams.from_buffer_copy(self)
        sp.N = self.P * 256
        return sp


@N.params_of("HZ_K_SEARCH_QLSCAN")
class QuantListScanParams(C.Structure):
    """HzSearchQuantListParams: the fields of ``ListScanParams`` (``corpus``: uint8 rows, ``ldc`` in bytes), then
    ``scales`` (fp32 [N] in stored order)."""
    _fields_ = ListScanParams._fields_ + [("scales", C.c_void_p)]

    def merge_params(self) -> SearchParams:
        sp = SearchParams.from_buffer_copy(self)
        sp.N = self.P * 256
        return sp


@N.params_of("HZ_K_SEARCH_MERGEN")
@N.params_of("HZ_K_SEARCH_MSCAN")
class SelfScanParams(C.Structure):
    """HzSearchSelfParams: ``corpus`` bf16 [N][ldc], ``qid`` device int32 [Q] (the rows that are the queries), the
    required ``live`` bitmap, ``cand`` [ntile][Q][k] keys, the merge's outputs [Q][k], then the byte counts and shape."""
    _fields_ = [("corpus", C.c_void_p), ("qid", C.c_void_p), ("live", C.c_void_p), ("cand", C.c_void_p),
                ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("live_bytes", C.c_uint64), ("cand_bytes", C.c_uint64),
                ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int), ("ldc", C.c_int), ("ntile", C.c_int),
                ("skip_self", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_SEARCH_XSCAN")
class BatchScanParams(C.Structure):
    """HzSearchBatchParams: ``SelfScanParams`` with ``queries`` (device fp32 [Q][D], 16-B aligned) where ``qid`` is and
    two unused ints where ``skip_self`` is -- the same layout, so ``HZ_K_SEARCH_MERGEN`` takes it as it stands."""
    _fields_ = [("corpus", C.c_void_p), ("queries", C.c_void_p), ("live", C.c_void_p), ("cand", C.c_void_p),
                ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("live_bytes", C.c_uint64), ("cand_bytes", C.c_uint64),
                ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int), ("ldc", C.c_int), ("ntile", C.c_int),
                ("pad_", C.c_int * 2)]

    def merge_params(self) -> SelfScanParams:
        """The block as ``HZ_K_SEARCH_MERGEN`` reads it."""
        return SelfScanParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_ASSIGN")
class AssignParams(C.Structure):
    """HzSearchAssignParams: ``corpus`` bf16 [N][ldc], ``cent`` bf16 [C][ldk], the required ``live`` bitmap (any
    bitmap: a row without its bit gets -1 / -inf), ``out_list`` int32 [N], ``out_score`` fp32 [N]."""
    _fields_ = [("corpus", C.c_void_p), ("cent", C.c_void_p), ("live", C.c_void_p), ("out_list", C.c_void_p),
                ("out_score", C.c_void_p), ("live_bytes", C.c_uint64), ("N", C.c_int), ("D", C.c_int), ("C", C.c_int),
                ("ldc", C.c_int), ("ldk", C.c_int), ("ntile", C.c_int)]


@N.params_of("HZ_K_SEARCH_CMEAN")
class CmeanParams(C.Structure):
    """HzSearchCmeanParams: ``order`` device int32 [M] (the members' row ids, cluster after cluster), ``seg_off`` device
    int32 [C + 1], ``cent`` bf16 [C][ldk] in and out, ``cent32`` fp32 [C][D] out or null."""
    _fields_ = [("corpus", C.c_void_p), ("order", C.c_void_p), ("seg_off", C.c_void_p), ("cent", C.c_void_p),
                ("cent32", C.c_void_p), ("N", C.c_int), ("D", C.c_int), ("C", C.c_int), ("M", C.c_int), ("ldc", C.c_int),
                ("ldk", C.c_int), ("cosine", C.c_int), ("pad_", C.c_int)]


def _sigs(lib):
    P, U64 = C.c_void_p, C.c_uint64
    N._sig(lib, "hz_search_assign_launch", C.c_int, C.POINTER(AssignParams), P)
    N._sig(lib, "hz_search_cmean_launch", C.c_int, C.POINTER(CmeanParams), P)
    N._sig(lib, "hz_index_assign", C.c_int, P, C.c_int, P, C.c_int, P, P, P)
    N._sig(lib, "hz_index_cmean", C.c_int, P, C.c_int, P, C.c_longlong, P, C.c_int, P, P)
    N._sig(lib, "hz_search_self_scratch_bytes", U64, C.c_longlong, C.c_longlong, C.c_int)
    N._sig(lib, "hz_search_mscan_launch", C.c_int, C.POINTER(SelfScanParams), P)
    N._sig(lib, "hz_search_mergen_launch", C.c_int, C.POINTER(SelfScanParams), P)
    N._sig(lib, "hz_search_xscan_launch", C.c_int, C.POINTER(BatchScanParams), P)
    N._sig(lib, "hz_search_rescoren_launch", C.c_int, C.POINTER(RescoreParams), P)
    N._sig(lib, "hz_index_search_batch", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_index_neighbors", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_neighbors_max", C.c_int, P, C.c_int)
    N._sig(lib, "hz_search_tile_rows", C.c_int)
    N._sig(lib, "hz_search_scratch_bytes", U64, C.c_longlong, C.c_int, C.c_int)
    N._sig(lib, "hz_search_scan_launch", C.c_int, C.POINTER(SearchParams), P)
    N._sig(lib, "hz_search_merge_launch", C.c_int, C.POINTER(SearchParams), P)
    N._sig(lib, "hz_search_fscan_launch", C.c_int, C.POINTER(FilterScanParams), P)
    N._sig(lib, "hz_search_qscan_launch", C.c_int, C.POINTER(QuantScanParams), P)
    N._sig(lib, "hz_search_rescore_launch", C.c_int, C.POINTER(RescoreParams), P)
    N._sig(lib, "hz_search_bscan_launch", C.c_int, C.POINTER(BinScanParams), P)
    N._sig(lib, "hz_index_add_b", C.c_int, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_add_br", C.c_int, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_state_b", C.c_int, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_search_pqlut_launch", C.c_int, C.POINTER(PqLutParams), P)
    N._sig(lib, "hz_search_pqscan_launch", C.c_int, C.POINTER(PqScanParams), P)
    N._sig(lib, "hz_search_pq_span", C.c_int, C.c_longlong, C.c_int, C.c_int)
    N._sig(lib, "hz_search_pqassign_launch", C.c_int, C.POINTER(PqAssignParams), P)
    N._sig(lib, "hz_pq_encode", C.c_int, C.c_int, P, C.c_longlong, C.c_int, C.c_int, P, C.c_longlong, P, P)
    N._sig(lib, "hz_index_add_p", C.c_int, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_add_pr", C.c_int, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_state_p", C.c_int, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_read_codebook", C.c_int, P, P)
    N._sig(lib, "hz_index_describe4", C.c_int, P, C.POINTER(U64))
    N._sig(lib, "hz_search_lscan_launch", C.c_int, C.POINTER(ListScanParams), P)
    N._sig(lib, "hz_search_qlscan_launch", C.c_int, C.POINTER(QuantListScanParams), P)
    N._sig(lib, "hz_search_code_warm", C.c_int)
    N._sig(lib, "hz_index_last_error", C.c_char_p)
    N._sig(lib, "hz_index_open", P, C.c_char_p, C.c_int, C.c_int)
    N._sig(lib, "hz_index_describe", C.c_int, P, C.POINTER(U64))
    N._sig(lib, "hz_index_search", C.c_int, P, C.c_int, P, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_close", None, P)
    N._sig(lib, "hz_index_open2", P, C.c_char_p, C.c_int, C.c_int, C.c_longlong)
    N._sig(lib, "hz_index_describe2", C.c_int, P, C.POINTER(U64))
    N._sig(lib, "hz_index_search_filtered", C.c_int, P, C.c_int, P, P, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_add", C.c_int, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_delete", C.c_int, P, P, C.c_longlong, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_set_tags", C.c_int, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_read_state", C.c_int, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_add_q", C.c_int, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_state_q", C.c_int, P, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_open3", P, C.c_char_p, C.c_int, C.c_int, C.c_longlong, C.c_int)
    N._sig(lib, "hz_index_search2", C.c_int, P, C.c_int, P, P, C.c_int, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_add_qr", C.c_int, P, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_rescore", C.c_int, P, P, C.c_longlong)
    N._sig(lib, "hz_index_search3", C.c_int, P, C.c_int, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_probes", C.c_int, P, C.c_int, P, C.c_int, C.c_int, P)
    N._sig(lib, "hz_index_describe3", C.c_int, P, C.POINTER(U64))


N._EXTRA_SIGS.append(_sigs)
if N._lib is not None:  # the library was loaded before this module
    _sigs(N._lib)


def tile_rows() -> int:
    """Corpus rows per scan workgroup (a tile)."""
    return int(N.lib().hz_search_tile_rows())


def scratch_bytes(n: int, q: int, k: int) -> int:
    """Bytes of candidate scratch a search of (N, Q, k) needs; 0 for a refused shape."""
    return int(N.lib().hz_search_scratch_bytes(int(n), int(q), int(k)))


def launch(prm: SearchParams, stream: int = 0) -> tuple:
    """Scan then merge on ``stream``: (scan code, merge code); the merge is not launched after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_scan_launch(C.byref(prm), stream)
    return rc, (lib.hz_search_merge_launch(C.byref(prm), stream) if rc == 0 else None)


def launch_filtered(prm: FilterScanParams, stream: int = 0) -> tuple:
    """Filtered scan then merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_fscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def launch_quant(prm: QuantScanParams, stream: int = 0) -> tuple:
    """Quantised scan then merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_qscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def launch_bin(prm: BinScanParams, stream: int = 0) -> tuple:
    """Binary scan then merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_bscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def launch_pq_lut(prm: PqLutParams, stream: int = 0) -> int:
    """The table launch (``HZ_K_SEARCH_PQLUT``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_pqlut_launch(C.byref(prm), stream))


def launch_pq(prm: PqScanParams, stream: int = 0) -> tuple:
    """Product-quantised scan (over a table ``launch_pq_lut`` wrote) then merge on ``stream``: (scan code, merge
    code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_pqscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def pq_span(n: int, q: int, m: int) -> int:
    """The tiles per workgroup a scan of (N, Q) over rows of M codes takes with ``span`` = 0 on the current device; 0
    for a refused shape."""
    return int(N.lib().hz_search_pq_span(int(n), int(q), int(m)))


def launch_pq_assign(prm: PqAssignParams, stream: int = 0) -> int:
    """The assign launch (``HZ_K_SEARCH_PQASSIGN``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_pqassign_launch(C.byref(prm), stream))


def pq_encode_rows(bits, codebook, *, device: int = 0, chunk_rows: int = 0, want_dist: bool = False):
    """``hz_pq_encode``: bf16 rows ``bits`` (uint16 [n, D], host) against ``codebook`` (fp32 [M, 256, D / M], host) on
    ``device`` -> (codes uint8 [n, M], dist fp32 [n, M] or None). ``chunk_rows``: rows per device pass, 0 for the
    default. A refused shape is a ValueError with the launcher's code, a device failure a RuntimeError."""
    import numpy as np
    bits = np.ascontiguousarray(bits, np.uint16)
    cb = np.ascontiguousarray(codebook, np.float32)
    if bits.ndim != 2 or cb.ndim != 3 or cb.shape[1] != PQ_KSUB or cb.shape[0] * cb.shape[2] != bits.shape[1]:
        raise ValueError(f"rows must be uint16 [n, D] and the codebook fp32 [M, {PQ_KSUB}, D / M], got {list(bits.shape)} "
                         f"and {list(cb.shape)}")
    n, d = bits.shape
    m = cb.shape[0]
    codes = np.empty((n, m), np.uint8)
    dist = np.empty((n, m), np.float32) if want_dist else None
    lib = N.lib()
    rc = int(lib.hz_pq_encode(int(device), bits.ctypes.data, n, d, m, cb.ctypes.data, int(chunk_rows), codes.ctypes.data,
                              dist.ctypes.data if want_dist else None))
    if rc:
        msg = (lib.hz_index_last_error() or b"").decode()
        if rc in (-140, -141):
            raise (ValueError if rc == -141 else RuntimeError)(msg or f"hz_pq_encode failed ({rc})")
        raise ValueError(f"hz_pq_encode refused n = {n}, dim = {d}, m = {m} ({rc}: csrc/hipzap.h HZ_K_SEARCH_PQASSIGN)")
    return codes, dist


def launch_rescore(prm: RescoreParams, stream: int = 0) -> int:
    """The rescore launch on ``stream`` -> its code (0, or negative for a refused block: nothing ran)."""
    return int(N.lib().hz_search_rescore_launch(C.byref(prm), stream))


def launch_list(prm: ListScanParams, stream: int = 0) -> tuple:
    """List scan then merge (over the P candidate lists) on ``stream``: (scan code, merge code); no merge after a
    refused scan."""
    lib = N.lib()
    rc = lib.hz_search_lscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.merge_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def launch_quant_list(prm: QuantListScanParams, stream: int = 0) -> tuple:
    """Quantised list scan then merge (over the P candidate lists) on ``stream``: (scan code, merge code); no merge
    after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_qlscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.merge_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def self_scratch_bytes(n: int, q: int, k: int) -> int:
    """Bytes of candidate scratch a self scan of (N, Q, k) needs; 0 for a refused shape."""
    return int(N.lib().hz_search_self_scratch_bytes(int(n), int(q), int(k)))


def launch_self(prm: SelfScanParams, stream: int = 0) -> tuple:
    """Self scan then its merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_mscan_launch(C.byref(prm), stream)
    return rc, (lib.hz_search_mergen_launch(C.byref(prm), stream) if rc == 0 else None)


def launch_batch(prm: BatchScanParams, stream: int = 0) -> tuple:
    """Batch scan then ``HZ_K_SEARCH_MERGEN`` over the same block on ``stream``: (scan code, merge code); no merge after
    a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_xscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    mp = prm.merge_params()
    return rc, lib.hz_search_mergen_launch(C.byref(mp), stream)


def launch_rescore_n(prm: RescoreParams, stream: int = 0) -> int:
    """The rescore launch for any number of queries (``HZ_K_SEARCH_RESCOREN``) on ``stream`` -> its code."""
    return int(N.lib().hz_search_rescoren_launch(C.byref(prm), stream))
